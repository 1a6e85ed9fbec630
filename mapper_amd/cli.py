"""Command-line harness in the shape of `java -jar x-mapper.jar` (Mapper.main, Mapper.java:37-453; Mapper.run :639-812) for the part
of it that this repository accelerates: reference + queries in, alignments out as SAM.

    python -m mapper_amd --reference ref.fasta --queries reads.fastq --out-sam out.sam
    python -m mapper_amd --reference ref.fasta --paired-queries r1.fq r2.fq --spacing 100 50 --out-sam out.sam --out-unaligned un.fasta

SURVEY.md section 8(f) rank 1.  What is pinned by the reference: the flag names and their defaults (Mapper.java:82-453), the
derivation of AlignmentParameters from them (:409-453), reference sorting (:1151-1172), the SAM record format
(SamWriter_Test.java) and the statistics lines of Mapper.run (:786-796).  The SAM header, `--out-unaligned` and the other writers
live in the un-vendored QuickVariants module: the header written here is the minimal SAM-spec one and is marked [unpinned]; the
VCF / ancestry outputs stay with the Java host (`--cache-dir` is
honoured: the index goes to one file under it, api.index_cache_path) and are refused here with a message saying so.

Flags of this harness that Mapper does not have: --batch-size <n>, --gpus <n>, --contexts <n>, --devices <i,j,...>, --device <i>, --per-object,
--collapse-identical-queries (byte-identical queries of a batch are aligned once and share the results, as the reference's alignment cache does; the
outputs are the same, and one line on stderr says how many queries were served as copies), --remember-queries <MiB> (every context keeps the queries
it has aligned in that much HBM and serves byte-identical queries of its later batches from there: the same cache across batches; same outputs, one line on
stderr), and --remember-queries-per-gpu <MiB> (one such memory per GPU, which all its contexts share and which keeps remembering when it is full; not
together with --remember-queries), and --parse-on-gpu (the FASTQ files go to the GPU as text and are parsed there, api.ReferenceDatabase.stage_fastq: same outputs;
four-line FASTQ records only, so a file the host reader takes may be refused with a message that says where; not with --per-object, and with a split size
only beside --split-on-gpu; a job whose output needs objects - --out-refs-map-count without --count-refs-on-gpu, needs_objects - parses on the host all the
same), --split-on-gpu (with --parse-on-gpu and --split-queries-past-size: the kernels that parse the text also cut every record into its sections,
hostio.read_text_blocks(split=...), so a long-read job goes from FASTQ text to SAM text without the host translating or cutting a base; a record's sections
stay in one batch, where the host reader lets them straddle two; SAM, unaligned file, refs count and statistics are the same bytes at any --batch-size, the
mutations file where both paths cut their batches at the same places), --fasta-on-gpu (with --parse-on-gpu: a query file whose first record is FASTA -
'>', records of any number of lines - is parsed on the GPU too, hostio.read_text_blocks(fasta=True) and xm_batch_stage_fasta; same outputs, the unaligned
file being FASTA as the host writes it for mates without quality; without the flag such a file is refused as before; the two files of a pair must be of
one format; works beside --split-on-gpu and the other device stages),
--format-on-gpu (the SAM records are formatted on the GPU while a batch and its results are resident, api.ReferenceDatabase.format_sam_last, and the host
only writes the bytes: same outputs; --out-unaligned stays with the host; not with --per-object, --out-mutations or --out-refs-map-count; nothing to do
without --out-sam), --results-on-gpu (the align calls leave their result streams in HBM and copy none of them to the host,
api.ReferenceDatabase.set_result_copy(False); what the host still needs of them - the statistics, every alignment's penalty, the unaligned queries - is computed
on the GPU while the batch is resident, api.ReferenceDatabase.summary_last: same outputs; with --out-sam only together with --format-on-gpu, since the host
formatter reads the streams; fine with --out-unaligned, --no-output and --out-mutations, whose pile-up reads the resident streams; not with --per-object or
--out-refs-map-count, which decode the streams on the host - unless the count is made on the GPU, next), --count-refs-on-gpu (the count behind
--out-refs-map-count is made on the GPU while a batch and its results are resident, api.ReferenceDatabase.refs_count_last: per batch the queries per
combination of contigs cross to the host, and the job needs no objects: it streams like any other, parses on the GPU if --parse-on-gpu says so, and
--out-refs-map-count is then accepted beside --format-on-gpu and --results-on-gpu; same file; not with --per-object; nothing to do without
--out-refs-map-count), --unaligned-on-gpu (the unaligned-query file's text is made on the GPU while a batch and its results are resident,
api.ReferenceDatabase.unaligned_format_last, and the host only writes the bytes: same file; needs --out-unaligned, --parse-on-gpu - the names and qualities
are then in HBM with the batch - and --results-on-gpu, whose summary the statistics come from), --batch-on-gpu (a batch parsed on the GPU stays there: of
what the kernels build only the mate counts, offsets and lengths are copied to the host, api.ReferenceDatabase.set_batch_copy(False); same outputs; needs
--parse-on-gpu and --results-on-gpu, since the host's formatter and writers read the batch, and with --out-unaligned also --unaligned-on-gpu; not with
--per-object), --call-mutations-on-gpu (the end of --out-mutations runs where the pile-up lies: the replicas' counts are summed on the GPU, the SNP rows are
picked there and the indel candidates judged there, pileup.MatchDatabase.mutations(on_gpu=True), so that only the rows cross to the host and not 40 to 48 bytes
per reference base and context; same file; needs --out-mutations; not with --per-object; beside it --format-on-gpu is accepted with --out-mutations), --group-indels-on-gpu (the
pile-up's insertion / deletion events are grouped on the GPU as the batches come in, pileup.MatchDatabase(group_on_gpu=True): a table of groups per context in
HBM takes the place of the events that every batch copied to the host and that the host held to the end of the job and grouped one by one; same file; needs
--out-mutations; not with --per-object; independent of --call-mutations-on-gpu, beside which only the groups that pass the thresholds cross to the host),
and --format-threads <n> (threads of the host's SAM formatter).

--out-mutations streams like --out-sam: the device pile-up keeps the bases of every insertion with its event (pileup.MatchDatabase(keep_insert_text=True)), so
the mutations file needs no object per read; with --per-object it is written the first way, from the Query objects of the whole job, which is the reference
the streamed one is compared with.
"""
import contextlib
import gzip
import itertools
import queue
import sys
import threading
import time

import numpy as np

from . import api, hostio, sam

JAVA_HOST_ONLY = {"--out-vcf": 1, "--out-ancestor": 1, "--infer-ancestors": 0, "--verify-consistent-db": 0,
                  "--vcf-exclude-non-mutations": 0, "--vcf-omit-support-reads": 0}
IGNORED = {"--verbose": 0, "-v": 0, "-vv": 0, "--verbose-alignment": 0, "--verbose-reference": 0, "--verbosity-auto": 0, "--num-threads": 1,
           "--no-infer-ancestors": 0, "--allow-duplicate-contig-names": 0, "--version": 0}


class UsageError(Exception):
    pass


last_timing = None  # run: queries, seconds and contexts of the last job's streaming phase (bench.py's end_to_end leg)


def _open(path):
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path, "r")


def read_sequences(path):
    """FASTA or FASTQ (optionally .gz) -> list of (name, text, quality or None).  The name is the header up to the first blank."""
    out = []
    with _open(path) as f:
        lines = f.read().splitlines()
    i, n = 0, len(lines)
    while i < n:
        line = lines[i].rstrip("\r")
        if not line:
            i += 1
            continue
        if line[0] == ">":
            name = line[1:].split()[0] if len(line) > 1 else ""
            i += 1
            parts = []
            while i < n and not lines[i].startswith(">"):
                parts.append(lines[i].strip())
                i += 1
            out.append((name, "".join(parts).upper(), None))
        elif line[0] == "@":
            name = line[1:].split()[0] if len(line) > 1 else ""
            seq = lines[i + 1].strip().upper()
            qual = lines[i + 3].strip() if i + 3 < n else ""
            i += 4
            out.append((name, seq, qual))
        else:
            raise ValueError("%s: line %d is neither a FASTA nor a FASTQ header" % (path, i + 1))
    return out


def parse_args(argv):
    """Mapper.main's flag loop (Mapper.java:82-385) for the flags of this path."""
    o = dict(references=[], queries=[], paired=[], out_sam=None, out_unaligned=None, no_output=False, enable_gapmers=True,
             mutationPenalty=-1.0, indelStart_penalty=1.5, indelExtension_penalty=0.5, additional_insertionExtension_penalty=-1.0,
             maxErrorRate=-1.0, ambiguityPenalty=-1.0, maxNumMatches=2**31 - 1, max_penaltySpan=-1.0, device=0,
             paired_without_spacing=False, help=False, split=0)
    i = 0
    while i < len(argv):
        a = argv[i]
        if a == "--help":
            o["help"] = True
        elif a == "--reference":
            o["references"].append(argv[i + 1]); i += 1
        elif a == "--queries":
            o["queries"].append((argv[i + 1], o["split"])); i += 1
        elif a == "--split-queries-past-size":  # Mapper.java:142-148: applies to the --queries that follow
            if o["queries"] or o["paired"]:
                raise UsageError("Sorry, --split-queries-past-size currently is only supported before --queries")
            o["split"] = int(argv[i + 1]); i += 1
        elif a == "--paired-queries":
            if o["split"] > 0:
                raise UsageError("Sorry, --paired-queries is not currently supported with --split-queries-past-size")
            left, right = argv[i + 1], argv[i + 2]
            i += 2
            expected, deviation = 100.0, 50.0  # Mapper.java:41-42
            if i + 1 < len(argv) and argv[i + 1] == "--spacing":
                expected, deviation = float(argv[i + 2]), float(argv[i + 3])
                i += 3
            else:
                o["paired_without_spacing"] = True
            o["paired"].append((left, right, expected, deviation))
        elif a == "--out-sam":
            o["out_sam"] = argv[i + 1]; i += 1
        elif a == "--out-unaligned":
            o["out_unaligned"] = argv[i + 1]; i += 1
        elif a == "--no-output":
            o["no_output"] = True
        elif a == "--no-gapmers":
            o["enable_gapmers"] = False
        elif a == "--new-indel-penalty":
            o["indelStart_penalty"] = float(argv[i + 1]); i += 1
        elif a == "--extend-indel-penalty":
            o["indelExtension_penalty"] = float(argv[i + 1]); i += 1
        elif a == "--additional-extend-insertion-penalty":
            o["additional_insertionExtension_penalty"] = float(argv[i + 1]); i += 1
        elif a == "--snp-penalty":
            o["mutationPenalty"] = float(argv[i + 1]); i += 1
            if o["mutationPenalty"] <= 0:
                raise UsageError("--snp-penalty must be > 0")
        elif a == "--max-penalty":
            o["maxErrorRate"] = float(argv[i + 1]); i += 1
            if o["maxErrorRate"] < 0:
                raise UsageError("--max-penalty must be >= 0")
        elif a == "--max-penalty-span":
            o["max_penaltySpan"] = float(argv[i + 1]); i += 1
            if o["max_penaltySpan"] < 0:
                raise UsageError("--max-penalty-span must be >= 0")
        elif a == "--ambiguity-penalty":
            o["ambiguityPenalty"] = float(argv[i + 1]); i += 1
            if o["ambiguityPenalty"] < 0:
                raise UsageError("--ambiguity-penalty must be >= 0")
        elif a == "--max-num-matches":
            o["maxNumMatches"] = int(argv[i + 1]); i += 1
        elif a == "--out-refs-map-count":  # Mapper.java:197: how many queries mapped to each combination of references
            o["out_refs_map_count"] = argv[i + 1]; i += 1
        elif a == "--out-mutations":  # Mapper.java:203-237: the mutations file (mapper_amd/pileup.py; accumulated on the GPU) and its nested thresholds
            o["out_mutations"] = argv[i + 1]; i += 1
            f = o.setdefault("mutation_filter", {})
            while i + 1 < len(argv):
                sub = argv[i + 1]
                if sub == "--snp-threshold":
                    f["minSNPTotalDepth"], f["minSNPDepthFraction"] = float(argv[i + 2]), float(argv[i + 3])
                elif sub == "--indel-start-threshold":
                    f["minIndelTotalStartDepth"], f["minIndelStartDepthFraction"] = float(argv[i + 2]), float(argv[i + 3])
                elif sub == "--indel-continue-threshold":
                    f["minIndelContinuationTotalDepth"], f["minIndelContinuationDepthFraction"] = float(argv[i + 2]), float(argv[i + 3])
                elif sub == "--indel-threshold":
                    f["minIndelTotalStartDepth"] = f["minIndelContinuationTotalDepth"] = float(argv[i + 2])
                    f["minIndelStartDepthFraction"] = f["minIndelContinuationDepthFraction"] = float(argv[i + 3])
                else:
                    break  # maybe this argument is a top-level argument
                i += 3
        elif a == "--distinguish-query-ends":  # Mapper.java:351-355
            o["query_end_fraction"] = float(argv[i + 1]); i += 1
            if not 0 <= o["query_end_fraction"] < 1:
                raise UsageError("--distinguish-query-ends must be >= 0 and < 1")
        elif a == "--cache-dir":  # Mapper.java:264: keep the hashed reference between runs
            o["cache_dir"] = argv[i + 1]; i += 1
        elif a == "--batch-size":  # (not a Mapper flag) queries per GPU batch; batches are streamed (upload of the next one during the alignment of the current one)
            o["batch_size"] = int(argv[i + 1]); i += 1
            if o["batch_size"] < 1:
                raise UsageError("--batch-size must be >= 1")
        elif a == "--gpus":  # (not a Mapper flag) align on GPUs 0..N-1: index replicated, batches dealt round-robin (mapper_amd/multi.py)
            o["gpus"] = int(argv[i + 1]); i += 1
            if o["gpus"] < 1:
                raise UsageError("--gpus must be >= 1")
        elif a == "--contexts":  # (not a Mapper flag) contexts per GPU: batches are aligned by several contexts of a GPU at the same time (fills idle wave slots)
            o["contexts"] = int(argv[i + 1]); i += 1
            if o["contexts"] < 1:
                raise UsageError("--contexts must be >= 1")
        elif a == "--devices":  # (not a Mapper flag) explicit GPU ordinals, comma-separated; an ordinal may repeat (two contexts on one GPU)
            o["devices"] = [int(x) for x in argv[i + 1].split(",")]; i += 1
        elif a == "--collapse-identical-queries":  # (not a Mapper flag) identical queries of a batch aligned once (api.ReferenceDatabase.set_collapse; AlignerWorker.java:264-291)
            o["collapse"] = True
        elif a == "--remember-queries":  # (not a Mapper flag) MiB of HBM per context for the queries it has aligned (api.ReferenceDatabase.set_memo): repeats in later batches are served from there
            o["remember"] = int(argv[i + 1]) << 20; i += 1
            if o["remember"] < 0:
                raise UsageError("--remember-queries must be >= 0")
        elif a == "--remember-queries-per-gpu":  # (not a Mapper flag) MiB of HBM per GPU for one memory of aligned queries that all contexts of the GPU share (api.QueryMemory): two generations, never full
            o["remember_per_gpu"] = int(argv[i + 1]) << 20; i += 1
            if o["remember_per_gpu"] < 0:
                raise UsageError("--remember-queries-per-gpu must be >= 0")
        elif a == "--per-object":  # (not a Mapper flag) the harness's first implementation: one Python object per read and per alignment (the reference for the formats; tests)
            o["per_object"] = True
        elif a == "--parse-on-gpu":  # (not a Mapper flag) the query files are cut into blocks of whole FASTQ records on the host and parsed on the GPU (api.ReferenceDatabase.stage_fastq)
            o["parse_on_gpu"] = True
        elif a == "--split-on-gpu":  # (not a Mapper flag) with --parse-on-gpu, the sections of --split-queries-past-size are cut on the GPU too (xm_fastq_text.split_past_size)
            o["split_on_gpu"] = True
        elif a == "--fasta-on-gpu":  # (not a Mapper flag) with --parse-on-gpu, query files whose first record is FASTA are parsed on the GPU as well (xm_batch_stage_fasta)
            o["fasta_on_gpu"] = True
        elif a == "--format-on-gpu":  # (not a Mapper flag) the SAM records are formatted on the GPU from the result streams while the batch is resident (api.ReferenceDatabase.format_sam_last)
            o["format_on_gpu"] = True
        elif a == "--results-on-gpu":  # (not a Mapper flag) the result streams stay in HBM; the host gets the SAM text and a summary (api.ReferenceDatabase.set_result_copy, summary_last)
            o["results_on_gpu"] = True
        elif a == "--count-refs-on-gpu":  # (not a Mapper flag) the count of --out-refs-map-count is made on the GPU from the resident result streams (api.ReferenceDatabase.refs_count_last)
            o["count_refs_on_gpu"] = True
        elif a == "--unaligned-on-gpu":  # (not a Mapper flag) the unaligned-query file's text is made on the GPU from the resident batch and streams (api.ReferenceDatabase.unaligned_format_last)
            o["unaligned_on_gpu"] = True
        elif a == "--batch-on-gpu":  # (not a Mapper flag) a batch parsed on the GPU stays in HBM: only the mate counts, offsets and lengths come down (api.ReferenceDatabase.set_batch_copy)
            o["batch_on_gpu"] = True
        elif a == "--call-mutations-on-gpu":  # (not a Mapper flag) the thresholds of --out-mutations are applied on the GPU, where the pile-up lies (pileup.MatchDatabase.mutations(on_gpu=True))
            o["call_mutations_on_gpu"] = True
        elif a == "--group-indels-on-gpu":  # (not a Mapper flag) the pile-up's insertion / deletion events are grouped on the GPU as the batches come in (pileup.MatchDatabase(group_on_gpu=True))
            o["group_indels_on_gpu"] = True
        elif a == "--format-threads":  # (not a Mapper flag) threads of the host's SAM formatter (hostio.Writer; default: the CPUs, 32 at the most)
            o["format_threads"] = int(argv[i + 1]); i += 1
            if o["format_threads"] < 1:
                raise UsageError("--format-threads must be >= 1")
        elif a == "--device":  # (not a Mapper flag) which GPU
            o["device"] = int(argv[i + 1]); i += 1
        elif a == "--spacing":
            raise UsageError("--spacing is not a top-level argument: try --paired-queries <queries> <queries2> --spacing <expected> <distancePerPenalty>")
        elif a in JAVA_HOST_ONLY:
            raise UsageError("%s is handled by the Java host (VCF / mutation / ancestry subsystems are outside the accelerated path, SURVEY.md section 8)" % a)
        elif a in IGNORED:
            i += IGNORED[a]
        else:
            raise UsageError("Unrecognized argument: " + a)
        i += 1
    if o.get("parse_on_gpu") and o.get("per_object"):
        raise UsageError("--parse-on-gpu and --per-object exclude each other (the per-object path reads the queries into Python objects)")
    if o.get("parse_on_gpu") and any(split > 0 for _, split in o["queries"]) and not o.get("split_on_gpu"):
        raise UsageError("--parse-on-gpu is not supported with --split-queries-past-size (the sections are cut by the host reader)")
    if o.get("split_on_gpu"):
        if not o.get("parse_on_gpu"):
            raise UsageError("--split-on-gpu needs --parse-on-gpu (the sections are cut by the kernels that parse the FASTQ text)")
        if not any(split > 0 for _, split in o["queries"]):
            raise UsageError("--split-on-gpu has nothing to do without --split-queries-past-size in front of --queries")
        if any(split > 30000 for _, split in o["queries"]):
            raise UsageError("--split-on-gpu takes a --split-queries-past-size of at most 30000 (a section is a mate)")
    if o.get("fasta_on_gpu") and not o.get("parse_on_gpu"):
        raise UsageError("--fasta-on-gpu needs --parse-on-gpu (it lets the kernels that parse the query text take FASTA records too)")
    if o.get("count_refs_on_gpu"):
        if o.get("per_object"):
            raise UsageError("--count-refs-on-gpu and --per-object exclude each other (the per-object path counts from alignments decoded on the host)")
        if not o.get("out_refs_map_count"):
            raise UsageError("--count-refs-on-gpu has nothing to do without --out-refs-map-count")
    if o.get("call_mutations_on_gpu"):
        if not o.get("out_mutations"):
            raise UsageError("--call-mutations-on-gpu has nothing to do without --out-mutations")
        if o.get("per_object"):
            raise UsageError("--call-mutations-on-gpu and --per-object exclude each other (the per-object path takes the text of insertions from Python objects; it is the reference the device path is compared with)")
    if o.get("group_indels_on_gpu"):
        if not o.get("out_mutations"):
            raise UsageError("--group-indels-on-gpu has nothing to do without --out-mutations")
        if o.get("out_refs_map_count") and not o.get("count_refs_on_gpu"):
            raise UsageError("--group-indels-on-gpu and --out-refs-map-count exclude each other without --count-refs-on-gpu (the count then runs the job through the per-object path)")
        if o.get("per_object"):
            raise UsageError("--group-indels-on-gpu and --per-object exclude each other (the per-object path takes the text of insertions from Python objects; the device groups the events with the text it keeps)")
    refs_need_objects = bool(o.get("out_refs_map_count") and not o.get("count_refs_on_gpu"))
    for other, key in (("--per-object", "per_object"), ("--out-mutations", "out_mutations"), ("--out-refs-map-count", "out_refs_map_count")):
        if key == "out_mutations" and o.get("call_mutations_on_gpu"):
            continue  # (with the mutations called on the GPU the pile-up has been run beside the device formatter: tests/test_gpu_mutations.py)
        if o.get("format_on_gpu") and o.get(key) and (key != "out_refs_map_count" or refs_need_objects):
            raise UsageError("--format-on-gpu and %s exclude each other (--per-object and --out-refs-map-count format on the host; the pile-up of --out-mutations has not been run beside the device formatter)" % other)
    if o.get("results_on_gpu"):
        if o.get("per_object"):
            raise UsageError("--results-on-gpu and --per-object exclude each other (the per-object path decodes the result streams on the host)")
        if refs_need_objects:
            raise UsageError("--results-on-gpu and --out-refs-map-count exclude each other (the count is made from alignments decoded on the host)")
        if o["out_sam"] and not o.get("format_on_gpu"):
            raise UsageError("--results-on-gpu with --out-sam needs --format-on-gpu (the host's SAM formatter reads the result streams, which stay on the GPU)")
    if o.get("unaligned_on_gpu"):
        if o.get("per_object"):
            raise UsageError("--unaligned-on-gpu and --per-object exclude each other (the per-object path writes the unaligned queries from Python objects)")
        if not o["out_unaligned"]:
            raise UsageError("--unaligned-on-gpu has nothing to do without --out-unaligned")
        if not o.get("parse_on_gpu"):
            raise UsageError("--unaligned-on-gpu needs --parse-on-gpu (the text is made from the names and qualities that the parser leaves in HBM with the batch)")
        if not o.get("results_on_gpu"):
            raise UsageError("--unaligned-on-gpu needs --results-on-gpu (the statistics then come from the summary, not from the host's walk that writes the unaligned queries)")
    if o.get("batch_on_gpu"):
        if o.get("per_object"):
            raise UsageError("--batch-on-gpu and --per-object exclude each other (the per-object path reads the queries into Python objects)")
        if not o.get("parse_on_gpu"):
            raise UsageError("--batch-on-gpu needs --parse-on-gpu (only a batch that the GPU parsed from text is there without a host copy)")
        if not o.get("results_on_gpu"):
            raise UsageError("--batch-on-gpu needs --results-on-gpu (the host's formatter walks the streams over the batch's arrays, which stay on the GPU)")
        if o["out_unaligned"] and not o.get("unaligned_on_gpu"):
            raise UsageError("--batch-on-gpu with --out-unaligned needs --unaligned-on-gpu (the host writes the unaligned queries from the batch's arrays, which stay on the GPU)")
    if o.get("remember") and o.get("remember_per_gpu"):
        raise UsageError("--remember-queries (a memory per context) and --remember-queries-per-gpu (one per GPU) exclude each other")
    return o


def derive_parameters(o):
    """Mapper.java:386-453: validation and the defaults that depend on other flags."""
    if len(o["references"]) < 1:
        raise UsageError("--reference is required")
    if len(o["queries"]) + len(o["paired"]) < 1:
        raise UsageError("--queries or --paired-queries is required")
    if o["out_sam"] is None and o["out_unaligned"] is None and not o.get("out_mutations") and not o.get("out_refs_map_count") and not o["no_output"]:
        raise UsageError("No output specified. Try --out-sam <output path>, or if you really don't want to generate an output file, --no-output")
    if o["maxErrorRate"] >= 0 and o["mutationPenalty"] >= 0 and o["paired_without_spacing"]:
        raise UsageError("Customized alignment penalties (--snp-penalty) and penalty threshold (--max-penalty) without customizing spacing penalty "
                         "between paired-end queries: please specify --spacing explicitly")
    maxErrorRate = o["maxErrorRate"] if o["maxErrorRate"] >= 0 else 0.1
    mutationPenalty = o["mutationPenalty"] if o["mutationPenalty"] > 0 else 1.0
    if o["indelExtension_penalty"] <= 0:
        raise UsageError("--extend-indel-penalty must be > 0")
    if o["indelStart_penalty"] <= 0:
        raise UsageError("--new-indel-penalty must be > 0")
    if o["maxNumMatches"] < 1:
        raise UsageError("--max-num-matches must be >= 1")
    span = o["max_penaltySpan"] if o["max_penaltySpan"] >= 0 else mutationPenalty / 2
    ambiguity = o["ambiguityPenalty"] if o["ambiguityPenalty"] >= 0 else maxErrorRate
    additional = o["additional_insertionExtension_penalty"] if o["additional_insertionExtension_penalty"] >= 0 else ambiguity
    return api.AlignmentParameters(MutationPenalty=mutationPenalty, DeletionStart_Penalty=o["indelStart_penalty"], DeletionExtension_Penalty=o["indelExtension_penalty"],
                                   InsertionStart_Penalty=o["indelStart_penalty"], InsertionExtension_Penalty=o["indelExtension_penalty"] + additional,
                                   MaxErrorRate=maxErrorRate, AmbiguityPenalty=ambiguity, UnalignedPenalty=ambiguity, MaxNumMatches=o["maxNumMatches"],
                                   Max_PenaltySpan=span)


def split_sections(length, max_length):
    """SequenceSplitter.java:9-38: a sequence longer than max_length becomes (length - 1) / max_length + 1 sections, section k covering
    [length * k / n, length * (k + 1) / n) (integer division in 64 bits, :35-38).  -> list of (start, end)."""
    num = (length - 1) // max_length + 1
    return [(length * k // num, length * (k + 1) // num) for k in range(num)]


def load_queries(o):
    """-> list of (api.Query, qualities or None) in input order: --queries files first, then --paired-queries files, as Mapper.main adds them."""
    out = []
    for path, split in o["queries"]:
        for name, text, qual in read_sequences(path):
            if split > 0:  # SequenceSplitter.java:9-40: equal sections of at most `split` bases (the sections carry no quality; their names are [unpinned])
                for a, b in split_sections(len(text), split):
                    out.append((api.Query(text[a:b], name=name), [None]))
            else:
                out.append((api.Query(text, name=name), [qual]))
    for left, right, expected, deviation in o["paired"]:
        ls, rs = read_sequences(left), read_sequences(right)
        if len(ls) != len(rs):
            raise UsageError("paired query files have different numbers of reads: %s %d, %s %d" % (left, len(ls), right, len(rs)))
        for (n1, t1, q1), (n2, t2, q2) in zip(ls, rs):
            out.append((api.Query(t1, t2, expected_inner_distance=expected, spacing_deviation_per_unit_penalty=deviation, names=[n1, n2]), [q1, q2]))
    return out


def java_float(x):
    """Float.toString of (float)x for the statistics lines: shortest decimal that round-trips the 32-bit value."""
    t = str(np.float32(x))
    return t if ("." in t or "e" in t or "n" in t) else t + ".0"


def sam_header(contigs):
    """[unpinned: SamWriter is un-vendored] minimal SAM-spec header: @HD, one @SQ per contig in the order of the reference files, @PG."""
    lines = ["@HD\tVN:1.6\tSO:unsorted"]
    lines += ["@SQ\tSN:%s\tLN:%d" % (name, len(text)) for name, text in contigs]
    lines.append("@PG\tID:xmapper-mi355x\tPN:xmapper-mi355x")
    return lines


def needs_objects(o):
    """Whether the job runs through the per-object path (object_source, ObjectSink): when it is asked for, and for the one output that is counted from
    decoded alignments, unless --count-refs-on-gpu has the GPU count it.  --out-mutations is not among them: its only use of the objects, the text of
    insertions, comes from the device pile-up."""
    return bool((o.get("out_refs_map_count") and not o.get("count_refs_on_gpu")) or o.get("per_object"))


def default_contexts(explicit_devices, batches, single_short):
    """Contexts per GPU for a job that does not say (--contexts): one where the GPUs are named (--devices, --gpus) and for a job of one batch.  A job of
    several batches gets two, which align their batches at the same time (+15-18 % reads per second on MI355X; on reads from i.i.d. references more contexts
    add nothing, profiles/r03/NOTES.md; on a repeat-rich reference, whose passes end with a long tail of few heavy reads, `--contexts 4` gives 1.45x over
    two, profiles/r04/NOTES.md 13).  single_short - every query a single read of up to 320 bases - in three batches or more: three contexts, each sized for
    a third of the GPU's wave slots, overlap best (+7 % over two, profiles/r04/NOTES.md 15; pairs and long reads are within 2 % from two to four contexts).
    Contexts share the index (xm_context_new), so a genome-sized one is no obstacle; they divide the HBM that is free once it is resident, and a GPU with
    room for fewer contexts uses fewer (api.divide_scratch)."""
    if explicit_devices or batches < 2:
        return 1
    return 3 if batches >= 3 and single_short else 2


def context_devices(o, batches, single_short):
    """-> the GPU ordinal of every context of the job: each GPU of --devices / --gpus (else --device) as often as it gets contexts."""
    explicit = o.get("devices") or (list(range(o["gpus"])) if o.get("gpus", 1) > 1 else None)
    contexts = o.get("contexts") or default_contexts(explicit is not None, batches, single_short)
    return [d for d in (explicit or [o["device"]]) for _ in range(contexts)]


def open_gpu_database(contigs, devices, max_query_length, enable_gapmers=True, collapse=False, cache_dir=None, per_context_extra=0, memo_bytes=0, shared_memo_bytes=0):
    """The index of `contigs` (in api.sort_reference order) with one context per entry of `devices`.  per_context_extra: what every context will allocate
    beside its scratch (api.divide_scratch; memo_bytes, every context's memory of aligned queries, is part of it; shared_memo_bytes, the one memory
    of each GPU, is not: it is counted once per GPU).  (A job whose later reads are longer than max_query_length grows the index on demand: xm_index_ensure_length.)"""
    if len(devices) > 1 or shared_memo_bytes:
        from . import multi
        return multi.MultiGpuDatabase(contigs, devices, collapse=collapse, memo_bytes=memo_bytes, shared_memo_bytes=shared_memo_bytes, mode="mapper", enable_gapmers=enable_gapmers, max_query_length=max_query_length,
                                      cache_dir=cache_dir, per_context_extra=per_context_extra)
    db = api.ReferenceDatabase(contigs, mode="mapper", enable_gapmers=enable_gapmers, device=devices[0], max_query_length=max_query_length, cache_dir=cache_dir)
    db.set_collapse(collapse)
    if memo_bytes:
        db.set_memo(memo_bytes)
    return db


def native_source(o, batch_size, job):
    """The query files parsed by libxm_hostio.so straight into batch arrays (hostio.Batch): no object per read, memory is O(batches in flight).  The reader
    cannot know the job's size, so the first batch speaks for the job: a full one counts as three batches or more, a short one as the only one.
    -> (batches, batch count for default_contexts, single_short, longest mate)"""
    keep_qual = bool(o["out_unaligned"])
    on_gpu = bool(o.get("parse_on_gpu"))  # the blocks are text (hostio.TextBlock) until a context stages them: the first one speaks through its longest line

    def is_fasta(*paths):
        """--fasta-on-gpu: do the files start with a FASTA record?  (Without the flag nothing is looked at: a '>' file is the FASTQ parser's to refuse, as before.)"""
        if not o.get("fasta_on_gpu"):
            return False
        first = [hostio.first_header_byte(p) for p in paths]
        if len(set(first) - {b""}) > 1:
            raise hostio.StrictFormError("paired query files are of different formats: %s" % ", ".join(
                "%s starts with a %s record" % (p, "FASTA" if c == b">" else "FASTQ") for p, c in zip(paths, first)))
        return b">" in first

    def read():
        if on_gpu:
            for path, split in o["queries"]:
                yield from hostio.read_text_blocks(path, None, batch_size, keep_qualities=keep_qual, split=split, fasta=is_fasta(path))  # (a split size: --split-on-gpu, parse_args)
            for left, right, expected, deviation in o["paired"]:
                yield from hostio.read_text_blocks(left, right, batch_size, keep_qualities=keep_qual, expected_inner=expected, deviation=deviation, fasta=is_fasta(left, right))
            return
        for path, split in o["queries"]:
            yield from hostio.read_batches(path, None, batch_size, split=split, keep_qualities=keep_qual)
        for left, right, expected, deviation in o["paired"]:
            yield from hostio.read_batches(left, right, batch_size, keep_qualities=keep_qual, expected_inner=expected, deviation=deviation)

    rest = read()
    job.callback(rest.close)  # (closes the query file the reader stands in)
    first = next(rest, None)
    if first is None:
        raise UsageError("no queries found")
    job.callback(first.close)
    max_len = max(first.longest_line, 1) if on_gpu else int(first.mate_length.max())
    single = not first.paired if on_gpu else int(first.mate_count.max()) == 1
    return itertools.chain([first], rest), 3 if len(first) >= batch_size else 1, single and max_len <= 320, max_len


@contextlib.contextmanager
def strict_form_hint():
    """--parse-on-gpu: a query file the device parser does not take ends the job with the library's message and the way out."""
    try:
        yield
    except hostio.StrictFormError as e:
        raise UsageError("%s; run without --parse-on-gpu" % e) from e


class ObjectBatch:
    """A slice of load_queries() in the shape of hostio.Batch."""

    def __init__(self, pairs):
        self.pairs = pairs
        self.queries = [q for q, _ in pairs]

    def arrays(self):
        return api.ReferenceDatabase.batch_arrays(self.queries)

    def __len__(self):
        return len(self.pairs)

    def close(self):
        pass


def object_source(o, batch_size):
    """--per-object, the harness's first implementation and the reference for the formats: one api.Query per read, all of them loaded before the first is
    aligned.  -> as native_source, from the real batch count and all queries."""
    pairs = load_queries(o)
    max_len = max([len(s) for q, _ in pairs for s in q.sequences] + [1])
    batches = [ObjectBatch(pairs[s:s + batch_size]) for s in range(0, len(pairs), batch_size)]
    return batches, len(batches), all(len(q.sequences) == 1 for q, _ in pairs) and max_len <= 320, max_len


def refs_map_key(indices, names):
    """The key of --out-refs-map-count for a query whose alignments lie on the contigs `indices`: a set over names, so contigs of one name merge."""
    return tuple(sorted({names[i] for i in indices}))


def write_refs_map(path, counts):
    """Mapper.java:747-756 (referenceAlignmentCounter.sumAlignments); [unpinned format]: one line per combination, most frequent first."""
    with open(path, "w") as f:
        for key, count in sorted(counts.items(), key=lambda kv: (-kv[1], kv[0])):
            f.write("%s\t%d\n" % (",".join(key), count))


class RefsTally:
    """--count-refs-on-gpu: the job's count per combination of contig names, added up batch by batch from what each context counted on its GPU.  add() runs in
    stream's on-context hook, on the replicas' threads: one counter, under a lock."""

    def __init__(self, names):
        self._names, self._lock, self.counts = names, threading.Lock(), {}

    def add(self, context):
        counted = context.refs_count_last()
        with self._lock:
            for indices, count in counted.items():
                key = refs_map_key(indices, self._names)
                self.counts[key] = self.counts.get(key, 0) + count


class ObjectSink:
    """hostio.Writer's job with one Python object per alignment (sam.records), plus the count behind --out-refs-map-count."""

    def __init__(self, contig_names, sam_file=None, unaligned_file=None, count_refs=False):
        self._names, self._sam, self._un = contig_names, sam_file, unaligned_file
        self.stats = hostio.XmioStats()
        self.refs_map = {} if count_refs else None

    def write(self, batch, result):
        st = self.stats
        for k, (q, quals) in enumerate(batch.pairs):
            comps = result.query_alignments(k)
            st.num_queries += 1
            if any(len(c) > 0 for c in comps):
                st.num_aligned += 1
                if self.refs_map is not None:  # ReferenceAlignmentCounter [QuickVariants, inferred]: the set of contigs a query's alignments lie on
                    key = refs_map_key((sa.contig for comp in comps for al in comp for sa in al.components), self._names)
                    self.refs_map[key] = self.refs_map.get(key, 0) + 1
                for comp in comps:  # AlignmentCounter [QuickVariants, inferred]: every reported alignment's aligned length, penalty and indels
                    for al in comp:
                        for sa in al.components:
                            st.total_aligned_length += sum(b.lengthA for b in sa.sections)
                            st.num_indels += sum(1 for b in sa.sections if b.lengthA != b.lengthB)
                        st.total_penalty += al.penalty
                if self._sam:
                    for line in sam.records(q, comps, self._names):
                        self._sam.write(line + "\n")
            elif self._un:  # [unpinned format] the query as it came in: FASTQ when it had qualities, else FASTA
                for name, seq, qual in zip(q.names, q.sequences, quals):
                    text = api.decode(seq)
                    self._un.write("@%s\n%s\n+\n%s\n" % (name, text, qual) if qual is not None else ">%s\n%s\n" % (name, text))

    def write_refs_map(self, path):
        write_refs_map(path, self.refs_map)


def stream(db, batches, params, sink, depth, on_aligned=None, tally=None, format_on_gpu=False, results_on_gpu=False, want_unaligned=False, refs_tally=None, unaligned_on_gpu=False):
    """The job: the batches stream through the GPU contexts (align_stream: the copy of batch k + 1 overlaps the alignment of batch k; several contexts align
    side by side) and a writer thread hands each batch and its result streams to the sink while the next batches are being aligned; at most `depth` results
    wait for it.  Every batch taken from `batches` is closed, and the first exception - the reader's, the GPU's or the sink's - reaches the caller.
    -> the queries that were served as copies (BatchResult.copies); tally["remembered"], if given, grows by the ones served from the contexts' memories
    (BatchResult.remembered).  format_on_gpu: the context that aligned a batch formats its SAM records while the batch is resident (format_sam_last, in the
    on_aligned hook: between two align calls of that context), and the writer thread writes the text; tally["read"] grows by the seconds the feeder waited for
    the reader.  results_on_gpu: the results carry no streams (set_result_copy(False) is the caller's); the same hook asks the context for the batch's summary
    (summary_last, with the list of unaligned queries if want_unaligned) behind the text and before the caller's on_aligned, and the summary travels to the
    writer thread with the text; both are closed there, also after a failure.  refs_tally (a RefsTally): the same hook has the context count the batch's queries
    per combination of contigs (refs_count_last) behind the text and the summary and before the caller's on_aligned.  unaligned_on_gpu (with results_on_gpu):
    the same hook asks the context for the text of the batch's unaligned queries (unaligned_format_last) behind the summary - which is then asked without the
    list - and before the caller's on_aligned; the text travels to the writer thread with the SAM text and the summary and is closed there, also after a failure."""
    in_flight = queue.Queue()  # batches in the order they were dealt to the GPUs
    to_write = queue.Queue(maxsize=depth)
    failure = []
    dealt, texts = {}, {}      # by batch number: the batch on its way to a context; [the text, the summary, the unaligned queries' text] its context made of it
    on_context = format_on_gpu or results_on_gpu or refs_tally is not None

    def feed():
        it = iter(batches)
        k = 0
        while True:
            t0 = time.perf_counter()
            b = next(it, None)
            if tally is not None:
                tally["read"] = tally.get("read", 0.0) + time.perf_counter() - t0
            if b is None:
                return
            in_flight.put(b)
            if on_context:
                dealt[k] = b
            k += 1
            yield b if isinstance(b, hostio.TextBlock) else b.arrays()  # (a text block is staged by the context that gets it: align_stream)

    hook = on_aligned
    if on_context:
        def hook(*at):  # ReferenceDatabase.align_stream calls it with (batch), MultiGpuDatabase's with (replica, batch), on the replica's thread
            b = dealt.pop(at[-1])
            context = db.replicas[at[0]] if len(at) > 1 else db
            made = texts[at[-1]] = [None, None, None]  # (registered first: what a failing call leaves behind is closed with the rest)
            if format_on_gpu:
                made[0] = context.format_sam_last(None if isinstance(b, hostio.TextBlock) else b)  # (a text block's names are in HBM with the batch)
            if results_on_gpu:
                made[1] = context.summary_last(want_unaligned=want_unaligned and not unaligned_on_gpu)
            if unaligned_on_gpu:
                made[2] = context.unaligned_format_last()
            if refs_tally is not None:
                refs_tally.add(context)
            if on_aligned is not None:
                on_aligned(*at)

    def write_loop():  # (after a failure it keeps taking what comes, unwritten, up to the end mark: the main thread never waits on a full queue for good)
        for b, r, made in iter(to_write.get, None):
            text, summary, unaligned = made or (None, None, None)
            try:
                if not failure:
                    sink.write(b, r, **({"sam_text": text} if text is not None else {}), **({"summary": summary} if summary is not None else {}),
                               **({"unaligned_text": unaligned} if unaligned is not None else {}))
            except BaseException as e:  # noqa: BLE001  (handed to the main thread)
                failure.append(e)
            finally:
                b.close()
                for held in (text, summary, unaligned):
                    if held is not None:
                        held.close()

    wt = threading.Thread(target=write_loop, daemon=True)
    wt.start()
    copies = 0
    results = db.align_stream(feed(), params, on_aligned=hook)
    try:
        for k, r in enumerate(results):
            if failure:
                break
            copies += r.copies
            if tally is not None:
                tally["remembered"] = tally.get("remembered", 0) + r.remembered
            to_write.put((in_flight.get(), r, texts.pop(k, None)))
    finally:
        to_write.put(None)
        wt.join()
        results.close()  # (ends the threads that deal and upload: nothing takes from `batches` after this)
        while not in_flight.empty():
            in_flight.get().close()
        for made in texts.values():
            for held in made:
                if held is not None:
                    held.close()
    if failure:
        raise failure[0]
    return copies


def write_statistics(out, st):
    """Mapper.run's statistics lines (Mapper.java:786-796) from the five numbers of hostio.XmioStats."""
    n = st.num_queries
    out.write("\nStatistics: \n")
    out.write(" Alignment rate                : %d%% of queries (%d/%d)\n" % (st.num_aligned * 100 // n if n else 0, st.num_aligned, n))
    if st.total_aligned_length:
        out.write(" Average penalty               : %s per base (%d/%d) in aligned queries\n" % (java_float(st.total_penalty / st.total_aligned_length), int(st.total_penalty), st.total_aligned_length))
        out.write(" Num indels                    : %s per base (%d/%d) in aligned queries\n" % (java_float(st.num_indels / st.total_aligned_length), st.num_indels, st.total_aligned_length))


def report_copies(copies, n):
    """--collapse-identical-queries: the one statistics line of the flag (stderr: the outputs stay what they are without it)."""
    sys.stderr.write("Identical queries: %d of %d queries were served as copies of an identical query of their batch\n" % (copies, n))


def report_remembered(remembered, n):
    """--remember-queries, --remember-queries-per-gpu: the one statistics line of the flag (stderr, like report_copies)."""
    sys.stderr.write("Remembered queries: %d of %d queries were served from an identical query of an earlier batch\n" % (remembered, n))


def run(argv, out=sys.stdout, open_database=None):
    """open_database: called as open_gpu_database is, in its place (tests hand in a database that needs no GPU)."""
    o = parse_args(argv)
    if o["help"] or not argv:
        out.write(__doc__ + "\n")
        return 0
    params = derive_parameters(o)
    contigs = []
    for path in o["references"]:
        contigs += [(name, text) for name, text, _ in read_sequences(path)]
    out.write("%d reference files:\n" % len(o["references"]))
    for path in o["references"]:
        out.write("Reference path = %s\n" % path)
    ordered = api.sort_reference(contigs)  # Mapper.sortAndComplementReference: alignment results refer to this order
    names = [n for n, _ in ordered]
    batch_size = o.get("batch_size") or 1_000_000
    per_object = needs_objects(o)
    with contextlib.ExitStack() as job:  # what the job opens is closed here, last opened first, also when a step raises
        job.enter_context(strict_form_hint())
        batches, count, single_short, max_len = object_source(o, batch_size) if per_object else native_source(o, batch_size, job)
        devices = context_devices(o, count, single_short)
        # (--out-mutations: every context accumulates its own pile-up on its GPU - depth 8 B, four alternative counts 32 B and, with a query-end fraction, the
        # middle depth 8 B per reference base: 149 GB for a 3.1 Gb reference - so the contexts of a GPU are counted with it)
        pile_up = (48 if o.get("query_end_fraction", 0.1) > 0 else 40) * sum(len(t) for _, t in ordered) + (64 << 20) if o.get("out_mutations") else 0
        # (--group-indels-on-gpu: the first allocation of a pile-up's table of groups, taken as an event per read - two to four slots of 16 bytes, a record
        # of 48, eight bytes of letters - and the arrays of a fold, a slot, four flags or lengths and two offsets per event; the table grows with the groups)
        if o.get("group_indels_on_gpu"):
            pile_up += batch_size * 192
        memo = {"memo_bytes": o["remember"]} if o.get("remember") else {}  # (--remember-queries: every context's memory, counted beside its scratch)
        if o.get("remember_per_gpu"):  # (--remember-queries-per-gpu: one memory per GPU, counted once per GPU when its contexts divide the scratch)
            memo = {"shared_memo_bytes": o["remember_per_gpu"]}
        # (--format-on-gpu: every context keeps the text of a batch in HBM, and per query two counts and an offset; a record is the mate's bases and name and
        # some 60 bytes of fields; with the host's names, those are copied up as well)
        format_on_gpu = bool(o.get("format_on_gpu") and o["out_sam"]) and not per_object  # (without --out-sam there is nothing to format)
        sam_text = batch_size * (2 * (max_len + 200) + 24) if format_on_gpu else 0
        # (--results-on-gpu: per query two counts and two offsets, and the penalties and the list, 8 bytes an alignment or an unaligned query)
        results_on_gpu = bool(o.get("results_on_gpu"))
        summary_arrays = batch_size * 64 if results_on_gpu else 0
        # (--count-refs-on-gpu: a table of two to four slots per query - key, first query and count, 24 bytes a slot - and per query a slot, three flags or
        # lengths and four offsets)
        refs_tally = RefsTally(names) if o.get("count_refs_on_gpu") else None
        refs_arrays = batch_size * 144 if refs_tally is not None else 0
        # (--unaligned-on-gpu: every context keeps the text of a batch's unaligned queries in HBM - at the most every mate's bases, qualities and name and six
        # bytes around them - and per query two counts, two offsets and an entry of the list)
        unaligned_on_gpu = bool(o.get("unaligned_on_gpu"))
        unaligned_text = batch_size * (2 * (2 * max_len + 200) + 32) if unaligned_on_gpu else 0
        db = (open_database or open_gpu_database)(ordered, devices, max_len, enable_gapmers=o["enable_gapmers"], collapse=o.get("collapse", False),
                                                  cache_dir=o.get("cache_dir"), per_context_extra=pile_up + o.get("remember", 0) + sam_text + summary_arrays + refs_arrays + unaligned_text, **memo)
        job.callback(db.close)
        if format_on_gpu:
            db.set_sam_contigs(names)
        if results_on_gpu:
            db.set_result_copy(False)
        if o.get("batch_on_gpu"):
            db.set_batch_copy(False)
        sam_out = un_out = None
        if o["out_sam"]:
            sam_out = sys.stdout if o["out_sam"] == "-" else job.enter_context(open(o["out_sam"], "w"))
            sam_out.write("\n".join(sam_header(contigs)) + "\n")
        if o["out_unaligned"]:
            un_out = job.enter_context(open(o["out_unaligned"], "w"))
        sink = ObjectSink(names, sam_out, un_out, bool(o.get("out_refs_map_count"))) if per_object else hostio.Writer(names, sam_out, un_out, threads=o.get("format_threads"))
        match_db = on_aligned = None
        if o.get("out_mutations"):  # Mapper.java:700-708: the MatchDatabase listens to every batch; here it accumulates on the GPU while the batch is resident
            from . import pileup
            # (default 0.1: Mapper.java:76; streamed batches are closed once they are written, so the pile-up keeps the text of insertions itself)
            grouping = {"group_on_gpu": True} if o.get("group_indels_on_gpu") else {}  # (--group-indels-on-gpu: the events are grouped where they lie)
            match_db = pileup.MatchDatabase(db.replicas if hasattr(db, "replicas") else db, o.get("query_end_fraction", 0.1), keep_insert_text=not per_object, **grouping)
            job.callback(match_db.close)

            def on_aligned(*at):  # ReferenceDatabase.align_stream calls it with (batch), MultiGpuDatabase's with (replica, batch), on the replica's thread
                match_db.add_last(batches[at[-1]].queries if per_object else None, replica=at[0] if len(at) > 1 else 0)
        t_stream = time.perf_counter()
        tally = {}
        copies = stream(db, batches, params, sink, 2 * len(devices), on_aligned, tally, format_on_gpu=format_on_gpu, results_on_gpu=results_on_gpu,
                        want_unaligned=bool(o["out_unaligned"]), refs_tally=refs_tally, unaligned_on_gpu=unaligned_on_gpu)
        contexts = list(getattr(db, "replicas", [db]))
        spent = lambda key: sum(getattr(c, "seconds", {}).get(key, 0.0) for c in contexts)  # noqa: E731
        # seconds of the job by phase, summed over batches (and over contexts, which work side by side: the sum may exceed the wall time): the reader or cutter,
        # staging (copy up, and the parse with --parse-on-gpu), the align calls, formatting SAM (on the host, or the GPU call with --format-on-gpu), file writes
        phases = {"read": tally.get("read", 0.0), "stage": spent("stage"), "align": spent("align"),
                  "format": spent("format") + getattr(sink, "seconds", {}).get("format", 0.0), "write": getattr(sink, "seconds", {}).get("write", 0.0)}
        if refs_tally is not None:
            write_refs_map(o["out_refs_map_count"], refs_tally.counts)
        elif o.get("out_refs_map_count"):
            sink.write_refs_map(o["out_refs_map_count"])
        if match_db is not None:  # Mapper.java:758-785
            with open(o["out_mutations"], "w") as f:
                filt = pileup.MutationDetectionParameters.defaultFilter()  # Mapper.java:56; --snp-threshold etc. override it
                for k, v in o.get("mutation_filter", {}).items():
                    setattr(filt, k, v)
                match_db.write_mutations(f, filt, on_gpu=bool(o.get("call_mutations_on_gpu")))
    n = int(sink.stats.num_queries)
    global last_timing
    last_timing = {"queries": n, "stream_seconds": time.perf_counter() - t_stream, "contexts": len(devices), "phases": phases}  # first batch to the GPUs .. last byte of the outputs (bench.py's end_to_end leg)
    if o.get("collapse"):
        report_copies(copies, n)
    if o.get("remember") or o.get("remember_per_gpu"):
        report_remembered(tally.get("remembered", 0), n)
    write_statistics(out, sink.stats)
    return 0


def main(argv=None):
    try:
        return run(sys.argv[1:] if argv is None else argv)
    except UsageError as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1


if __name__ == "__main__":
    sys.exit(main())
