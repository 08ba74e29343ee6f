"""The depth runs' contract, restated in numpy from a per-position array (include/callable_loci.h:
cl_contig_depth_runs; include/dut_coverage.h: dut_quantize_parse's bands and dut_depth_bed_write's text).  Nothing here
calls the library."""
import numpy as np


def values(depth, edges=None):
    """the depth itself, or with edges e_0 < e_1 < ... the number of edges <= depth"""
    depth = np.asarray(depth, np.uint64)
    if edges is None or len(edges) == 0:
        return depth
    return np.searchsorted(np.asarray(edges, np.uint64), depth, side="right").astype(np.uint64)


def runs(depth, edges=None):
    """depth: per-position depths of [0, extent) -> (start, value): a run starts at 0 and wherever the value differs from
    the one before; run i = [start[i], start[i + 1]), the last one ends at extent"""
    v = values(depth, edges)
    if v.shape[0] == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    start = np.flatnonzero(np.concatenate(([True], v[1:] != v[:-1])))
    return start.astype(np.uint32), v[start].astype(np.uint32)


def band(value, edges):
    lo = 0 if value == 0 else int(edges[value - 1])
    return "%d:%s" % (lo, "inf" if value == len(edges) else str(int(edges[value])))


def bed_text(contig, start, value, extent, edges=None):
    """contig, start, end, DEPTH -- or the band LO:HI with edges --, tab separated, no header"""
    lines = []
    for i in range(len(start)):
        end = int(start[i + 1]) if i + 1 < len(start) else int(extent)
        what = str(int(value[i])) if edges is None or len(edges) == 0 else band(int(value[i]), edges)
        lines.append("%s\t%d\t%d\t%s\n" % (contig, int(start[i]), end, what))
    return "".join(lines)


def bed_text_of(contig, depth, edges=None):
    s, v = runs(depth, edges)
    return bed_text(contig, s, v, len(depth), edges)


def parse(spec):
    """the edges of a --quantize argument: colon separated, a leading '0:' and a trailing ':' ignored"""
    if not spec:
        return []
    tok = spec.split(":")
    if len(tok) > 1 and tok[-1] == "":
        tok = tok[:-1]
    out = [int(t) for t in tok]
    return out[1:] if out and out[0] == 0 else out
