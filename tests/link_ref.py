"""An independent restatement of the linked-sites rule (cl_site_link_counts, dut_link_measure, dut_link_summarise and the
TSV of phase-sites), written from the rule of the README and not from csrc/link_walk.h: every read is first expanded into a
map position -> (class, quality value of the base that answers for it) by a CIGAR loop of its own, whatever sites are asked;
sites and pairs are then counted from those maps alone.  It never calls the engine and shares no code with the library."""
import bisect

import numpy as np

NONE = 255                                   # the quality value of a base without one: passes every threshold
CLASSES = ("A", "C", "G", "T", "del", "other")
DEL, OTHER = 4, 5
CODE_CLASS = {1: 0, 2: 1, 4: 2, 8: 3}


def expand(rec):
    """Per read its map {reference position: (class, quality value)}, its first reference position and one past its last."""
    maps, lo, hi = [], [], []
    for r in range(rec.n):
        x = int(rec.pos[r])
        s0, q0 = int(rec.seq_off[r]), int(rec.qual_off[r])
        L, nq = int(rec.seq_off[r + 1]) - s0, int(rec.qual_off[r + 1]) - q0
        lo.append(x)
        m = {}

        def code(q):
            b = int(rec.seq4[(s0 + q) >> 1])
            return b & 15 if (s0 + q) & 1 else b >> 4

        def qv(q):
            return int(rec.qual[q0 + q]) if q < nq else NONE

        y = 0
        for k in range(int(rec.cigar_off[r]), int(rec.cigar_off[r + 1])):
            w = int(rec.cigar[k])
            op, l = "MIDNSHP=X"[w & 15] if (w & 15) < 9 else "?", w >> 4
            if op in "M=X":
                for i in range(l):
                    if y + i < L:
                        m[x + i] = (CODE_CLASS.get(code(y + i), OTHER), qv(y + i))
                x += l; y += l
            elif op == "D":
                if 1 <= y <= L:                                            # the carrier: the stored base in front of the gap
                    for i in range(l):
                        m[x + i] = (DEL, qv(y - 1))
                x += l
            elif op == "N":
                x += l
            elif op in "IS":
                y += l
        maps.append(m); hi.append(x)
    return dict(maps=maps, lo=np.array(lo, np.int64), hi=np.array(hi, np.int64))


def pair_set(sites, max_dist, max_partners):
    """first (n + 1) of the pair set: anchor i with j = i + 1, ... while j <= i + max_partners and sites[j] - sites[i] <= max_dist."""
    first, n = [0], len(sites)
    for i in range(n):
        k = 0
        for j in range(i + 1, n):
            if j > i + max_partners or int(sites[j]) - int(sites[i]) > max_dist:
                break
            k += 1
        first.append(first[-1] + k)
    return np.array(first, np.uint32)


def counts(ev, rec, contig_len, sites, max_dist, max_partners, min_quality, exclude_flags=None, min_base_quality=None):
    """dict(first, tables (n_pairs, 6, 6), site_counts (n, 6)).  exclude_flags=None: no flag is read; min_base_quality (None:
    every base passes) holds only beside a mask."""
    sites = [int(s) for s in sites]
    first = pair_set(sites, max_dist, max_partners)
    n = len(sites)
    tables = np.zeros((int(first[n]), 6, 6), np.uint32)
    site_counts = np.zeros((n, 6), np.uint32)
    thr = min_base_quality if (exclude_flags is not None and min_base_quality is not None) else 0
    for r in range(rec.n):
        p0, p1 = int(ev["lo"][r]), int(ev["hi"][r])
        if not (0 <= p0 < contig_len) or int(rec.mapq[r]) < min_quality or p1 <= p0:
            continue
        if exclude_flags is not None and (int(rec.flag[r]) & exclude_flags):
            continue
        m = ev["maps"][r]

        def seen(p):
            o = m.get(p)
            return None if o is None or o[1] < thr else o[0]

        for i in range(bisect.bisect_left(sites, p0), bisect.bisect_left(sites, p1)):      # the anchors the read covers
            ca = seen(sites[i])
            if ca is None:
                continue
            site_counts[i, ca] += 1
            for k in range(int(first[i + 1]) - int(first[i])):
                cb = seen(sites[i + 1 + k])
                if cb is not None:
                    tables[int(first[i]) + k, ca, cb] += 1
    return dict(first=first, tables=tables, site_counts=site_counts)


def differences(got, want):
    """The names of the arrays in which a LinkResult (or a dict) differs from a dict of counts()."""
    get = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    return [k for k in ("first", "tables", "site_counts")
            if np.asarray(get(k)).shape != want[k].shape or not np.array_equal(np.asarray(get(k), np.uint32), want[k])]


STATUS = ("low_depth", "cis", "trans", "unresolved")


def summarise(ca, cb, table, min_depth, min_link_count, max_discord_per_10k):
    """The summary of one pair, in Python's integers: a dict with the columns of the TSV."""
    ca, cb, t = [int(v) for v in ca], [int(v) for v in cb], [[int(v) for v in row] for row in np.asarray(table).reshape(6, 6)]

    def two(c):
        major = max(range(5), key=lambda k: (c[k], -k))
        minor = max((k for k in range(5) if k != major), key=lambda k: (c[k], -k))
        return major, minor
    (Ma, ma), (Mb, mb) = two(ca), two(cb)
    both = sum(sum(row) for row in t)
    MM, Mm, mM, mm = t[Ma][Mb], t[Ma][mb], t[ma][Mb], t[ma][mb]
    n4, m = MM + Mm + mM + mm, Mm + mM + mm
    if n4 < min_depth:
        status = 0
    elif mm >= min_link_count and 10000 * (Mm + mM) <= max_discord_per_10k * m:
        status = 1
    elif Mm >= min_link_count and mM >= min_link_count and 10000 * mm <= max_discord_per_10k * m:
        status = 2
    else:
        status = 3
    return dict(status=status, major_a=Ma, minor_a=ma, major_b=Mb, minor_b=mb, depth_a=sum(ca), depth_b=sum(cb), both=both, MM=MM, Mm=Mm, mM=mM, mm=mm,
                other=both - n4)


def expected_tsv(contig, sites, res, sites_skipped=0, max_dist=1000, max_partners=4, min_depth=10, min_quality=20, min_link_count=3, max_discord_per_10k=500,
                 min_base_quality=None, exclude_flags=0):
    """The bytes of phase-sites for a dict of counts() over 0-based sites."""
    first, n_class, lines = res["first"], [0, 0, 0, 0], []
    for i in range(len(sites)):
        for p in range(int(first[i]), int(first[i + 1])):
            j = i + 1 + p - int(first[i])
            u = summarise(res["site_counts"][i], res["site_counts"][j], res["tables"][p], min_depth, min_link_count, max_discord_per_10k)
            n_class[u["status"]] += 1
            lines.append("\t".join([contig, str(int(sites[i]) + 1), str(int(sites[j]) + 1), str(int(sites[j]) - int(sites[i])), CLASSES[u["major_a"]], CLASSES[u["minor_a"]],
                                    CLASSES[u["major_b"]], CLASSES[u["minor_b"]]] + [str(u[k]) for k in ("depth_a", "depth_b", "both", "MM", "Mm", "mM", "mm", "other")] +
                                   [STATUS[u["status"]]]))
    head = (f"##contig={contig}\n##sites={len(sites)}\n##sites_skipped={sites_skipped}\n##pairs={int(first[len(sites)])}\n##max_dist={max_dist}\n"
            f"##max_partners={max_partners}\n##min_depth={min_depth}\n##min_quality={min_quality}\n"
            f"##min_base_quality={'.' if min_base_quality is None else min_base_quality}\n##exclude_flags=0x{exclude_flags:04x}\n"
            f"##min_link_count={min_link_count}\n##max_discordance={max_discord_per_10k / 10000:.4f}\n"
            f"##low_depth={n_class[0]}\n##cis={n_class[1]}\n##trans={n_class[2]}\n##unresolved={n_class[3]}\n"
            "#contig\tpos_a\tpos_b\tdist\tmajor_a\tminor_a\tmajor_b\tminor_b\tdepth_a\tdepth_b\tboth\tMM\tMm\tmM\tmm\tother\tstatus\n")
    return head + "".join(l + "\n" for l in lines)
