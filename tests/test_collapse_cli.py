"""CPU tier: the command line's --collapse-identical-queries (a flag of this harness, not of Mapper: identical queries of a batch aligned once)."""
import io

from mapper_amd import cli


def test_parse_args_records_the_flag():
    argv = ["--reference", "r.fa", "--queries", "q.fq", "--out-sam", "o.sam"]
    assert not cli.parse_args(argv).get("collapse")
    assert cli.parse_args(argv + ["--collapse-identical-queries"])["collapse"] is True
    assert cli.parse_args(["--collapse-identical-queries", "--batch-size", "10"] + argv)["batch_size"] == 10


def test_usage_lists_the_flag():
    out = io.StringIO()
    assert cli.run(["--help"], out=out) == 0
    assert "--collapse-identical-queries" in out.getvalue()
