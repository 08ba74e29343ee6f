"""An independent restatement of the error-profile rule (cl_site_error_profile, dut_error_profile_measure and the TSV of
error-profile), written from the rule of the README and not from csrc/ep_walk.h: every read is first expanded into one
record per base of its M/=/X operations (reference position, query index, 4-bit code, quality value) and one record per
insertion and deletion event (anchor or first deleted position, the query index that carries it, its length, that base's
quality value), whatever range is asked; a range is then counted from those records alone.  No interval arithmetic is
shared with the library."""
import numpy as np

NONE = 255                                   # the quality value of a base without one: passes every threshold
CELLS = [f + ">" + t for f in "ACGT" for t in "ACGT"]


def expand(rec):
    """dict(base=(r, p, q, code, qv), ins=(r, p, q, l, qv), dele=(r, p, q, l, qv), lo, hi, L) of numpy arrays: the records
    of every read of rec, and per read the first reference position, one past the last, and its stored base count."""
    base, ins, dele = [], [], []
    lo, hi, ls = [], [], []
    for r in range(rec.n):
        x = int(rec.pos[r])
        s0, q0 = int(rec.seq_off[r]), int(rec.qual_off[r])
        L, nq = int(rec.seq_off[r + 1]) - s0, int(rec.qual_off[r + 1]) - q0
        lo.append(x)

        def code(q):
            b = int(rec.seq4[(s0 + q) >> 1])
            return b & 15 if (s0 + q) & 1 else b >> 4

        def qv(q):
            return int(rec.qual[q0 + q]) if q < nq else NONE

        y, prev = 0, ("", 0)
        for k in range(int(rec.cigar_off[r]), int(rec.cigar_off[r + 1])):
            w = int(rec.cigar[k])
            op, l = "MIDNSHP=X"[w & 15] if (w & 15) < 9 else "?", w >> 4
            if op in "M=X":
                base += [(r, x + i, y + i, code(y + i), qv(y + i)) for i in range(l) if y + i < L]
                x += l; y += l
            elif op == "I":
                if prev[0] and prev[0] in "M=X" and prev[1] >= 1 and l >= 1 and y + l <= L:
                    ins.append((r, x - 1, y - 1, l, qv(y - 1)))
                y += l
            elif op == "D":
                if l >= 1 and 1 <= y <= L:
                    dele.append((r, x, y - 1, l, qv(y - 1)))
                x += l
            elif op == "N":
                x += l
            elif op == "S":
                y += l
            prev = (op, l)
        hi.append(x); ls.append(L)

    def cols(rows):
        a = np.array(rows, np.int64).reshape(-1, 5)
        return tuple(a[:, j] for j in range(5))
    return dict(base=cols(base), ins=cols(ins), dele=cols(dele), lo=np.array(lo, np.int64), hi=np.array(hi, np.int64), L=np.array(ls, np.int64))


REF_INDEX = np.full(256, 4, np.int64)
for _i, _c in enumerate("ACGT"):
    REF_INDEX[ord(_c)] = REF_INDEX[ord(_c.lower())] = _i
CODE_INDEX = np.full(16, 4, np.int64)
CODE_INDEX[[1, 2, 4, 8]] = [0, 1, 2, 3]


def profile(ev, rec, contig_len, ref, ref_len, start, end, n_cycles, min_quality, exclude_flags=None, min_base_quality=None):
    """The tables and scalars over [start, end) as a dict: total (4, 4), from5 / from3 (C, 4, 4), ins5 / ins3 / del5 / del3
    (C), reads, bases, uncomparable, ins, ins_bases, dels, del_bases.  exclude_flags=None: no flag is read and every read is
    forward; min_base_quality (None: every base passes) holds only beside a mask."""
    C = int(n_cycles)
    hi = min(int(end), int(ref_len))
    pos, flag = rec.pos.astype(np.int64), rec.flag.astype(np.int64)
    takes = (pos >= 0) & (pos < contig_len) & (rec.mapq.astype(np.int64) >= min_quality) & (ev["hi"] > ev["lo"]) & (ev["lo"] < hi) & (ev["hi"] > start)
    rev = np.zeros(rec.n, bool)
    if exclude_flags is not None:
        takes &= (flag & exclude_flags) == 0
        rev = (flag & 0x10) != 0
    thr = min_base_quality if (exclude_flags is not None and min_base_quality is not None) else 0
    ref = np.asarray(ref, np.uint8)
    out = dict(start=int(start), end=int(end), n_cycles=C, reads=int(takes.sum()) if start < hi else 0)

    def chosen(records):
        r, p, q, a, qv = records
        keep = takes[r] & (p >= start) & (p < hi) & (qv >= thr)
        r, p, q, a = r[keep], p[keep], q[keep], a[keep]
        d5 = np.where(rev[r], ev["L"][r] - 1 - q, q)
        return r, p, a, d5, ev["L"][r] - 1 - d5

    r, p, code, d5, d3 = chosen(ev["base"])
    f, t = REF_INDEX[ref[p]] if p.size else np.zeros(0, np.int64), CODE_INDEX[code]
    comparable = (f < 4) & (t < 4)
    out["uncomparable"] = int((~comparable).sum())
    r, f, t, d5, d3 = r[comparable], f[comparable], t[comparable], d5[comparable], d3[comparable]
    f, t = np.where(rev[r], 3 - f, f), np.where(rev[r], 3 - t, t)
    cell = 4 * f + t
    out["total"] = np.bincount(cell, minlength=16).astype(np.uint64).reshape(4, 4)
    out["bases"] = int(out["total"].sum())
    out["from5"] = np.bincount(d5[d5 < C] * 16 + cell[d5 < C], minlength=16 * C).astype(np.uint64).reshape(C, 4, 4)
    out["from3"] = np.bincount(d3[d3 < C] * 16 + cell[d3 < C], minlength=16 * C).astype(np.uint64).reshape(C, 4, 4)
    for name, n_name, b_name, records in (("ins", "ins", "ins_bases", ev["ins"]), ("del", "dels", "del_bases", ev["dele"])):
        r, p, l, d5, d3 = chosen(records)
        out[n_name], out[b_name] = int(r.size), int(l.sum())
        out[name + "5"] = np.bincount(d5[d5 < C], minlength=C).astype(np.uint64)
        out[name + "3"] = np.bincount(d3[d3 < C], minlength=C).astype(np.uint64)
    return out


SCALARS = ("start", "end", "n_cycles", "reads", "bases", "uncomparable", "ins", "ins_bases", "dels", "del_bases")
TABLES = ("total", "from5", "from3", "ins5", "ins3", "del5", "del3")


def differences(got, want):
    """The names of the scalars and tables in which an ErrorProfile (or a dict) differs from a dict of profile()."""
    get = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    bad = [k for k in SCALARS if int(get(k)) != int(want[k])]
    return bad + [k for k in TABLES if np.asarray(get(k)).shape != want[k].shape or not np.array_equal(np.asarray(get(k), np.uint64), want[k])]


def add(a, b):
    """Everything that is additive over a split range, of two dicts of profile(), as a dict without `reads`."""
    return {k: (a[k] + b[k]) for k in SCALARS[4:] + TABLES}


def rate(cells):
    cells = np.asarray(cells, np.uint64).reshape(16)
    n = int(cells.sum())
    return "NA" if n == 0 else "%.6f" % ((n - int(cells[0::5].sum())) / n)


def expected_tsv(contig, prof, min_quality, min_base_quality, exclude_flags):
    """The bytes of error-profile for a dict of profile()."""
    C = prof["n_cycles"]
    mism = prof["bases"] - int(np.asarray(prof["total"]).reshape(16)[0::5].sum())
    head = (f"##contig={contig}\n##range={prof['start']}-{prof['end']}\n##cycles={C}\n##min_quality={min_quality}\n"
            f"##min_base_quality={'.' if min_base_quality is None else min_base_quality}\n##exclude_flags=0x{exclude_flags:04x}\n"
            f"##reads={prof['reads']}\n##bases={prof['bases']}\n##uncomparable={prof['uncomparable']}\n##mismatches={mism}\n"
            f"##mismatch_rate={rate(prof['total'])}\n##insertions={prof['ins']}\n##inserted_bases={prof['ins_bases']}\n"
            f"##deletions={prof['dels']}\n##deleted_bases={prof['del_bases']}\n")
    lines = ["\t".join(["#table", "cycle"] + CELLS + ["ins", "del", "mismatch_rate"])]

    def line(table, cycle, cells, n_ins, n_del):
        lines.append("\t".join([table, cycle] + [str(int(v)) for v in np.asarray(cells).reshape(16)] + [str(int(n_ins)), str(int(n_del)), rate(cells)]))
    line("total", ".", prof["total"], prof["ins"], prof["dels"])
    for end5, tab, i_tab, d_tab in (("5p", "from5", "ins5", "del5"), ("3p", "from3", "ins3", "del3")):
        for d in range(C):
            line(end5, str(d + 1), prof[tab][d], prof[i_tab][d], prof[d_tab][d])
    return head + "\n".join(lines) + "\n"
