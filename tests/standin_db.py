"""A database for mapper_amd.cli.run that needs no GPU: the CPU oracle behind the part of ReferenceDatabase / MultiGpuDatabase the command line uses.

TEST INFRASTRUCTURE ONLY: handed to cli.run through its open_database keyword, so that the command-line pipeline - sources, hand-off, sinks, statistics -
runs in the CPU tier.  It takes cli.open_gpu_database's arguments, records them, and ignores the devices."""
import oracle_lib
from mapper_amd import api


class StandInDatabase:
    opened = []  # every instance, in the order they were made (a test clears it before its job)

    def __init__(self, contigs, devices, max_query_length, enable_gapmers=True, collapse=False, cache_dir=None, per_context_extra=0):
        self.oracle = oracle_lib.OracleReference(contigs, mode="mapper", enable_gapmers=enable_gapmers)
        self.devices, self.max_query_length, self.collapse, self.closed = list(devices), max_query_length, collapse, False
        StandInDatabase.opened.append(self)

    def set_collapse(self, enable):
        self.collapse = bool(enable)

    def align_stream(self, batches, parameters, on_aligned=None):
        p = parameters._c()  # (xm_params has the layout of oracle_lib.Params)
        for k, arrays in enumerate(batches):
            s = self.oracle.align(oracle_lib.QueryBatch.from_arrays(*arrays), p)
            if on_aligned is not None:
                on_aligned(k)
            yield api.BatchResult(dict(ints=s.ints, dbls=s.dbls, int_off=s.int_off, dbl_off=s.dbl_off, extra=[0] * 8))

    def close(self):
        self.closed = True
