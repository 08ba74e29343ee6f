"""fingerprint-compare restated in numpy, independent of the C code: a sketch is (hashes uint64 ascending, counts uint32,
ksize, scaled); a pair is compared over the entries with hash <= min(max_hash_a, max_hash_b)."""
import numpy as np

FIELDS = ("n_a", "n_b", "n_common", "sum_a", "sum_b", "sum_min")
HEADER = "#a\tb\tscaled\tn_a\tn_b\tcommon\tunion\tjaccard\tcontainment_a\tcontainment_b\tsum_a\tsum_b\tsum_min\tweighted_jaccard"


def max_hash(scaled):
    """((u64::MAX as f64) / scaled as f64) as u64 with a saturating cast: 2^64 / scaled in f64, floored."""
    if scaled <= 1:
        return 2 ** 64 - 1
    d = float(2 ** 64) / float(scaled)
    return min(int(d), 2 ** 64 - 1)


def compare_pair(a, b):
    """The six integers of one pair (Python ints)."""
    ha, ca, hb, cb = np.asarray(a[0], np.uint64), np.asarray(a[1], np.uint32), np.asarray(b[0], np.uint64), np.asarray(b[1], np.uint32)
    cut = np.uint64(min(max_hash(a[3]), max_hash(b[3])))
    na = int(np.searchsorted(ha, cut, side="right"))
    nb = int(np.searchsorted(hb, cut, side="right"))
    ha, ca, hb, cb = ha[:na], ca[:na], hb[:nb], cb[:nb]
    _, ia, ib = np.intersect1d(ha, hb, assume_unique=True, return_indices=True)
    smin = int(np.minimum(ca[ia], cb[ib]).astype(np.uint64).sum(dtype=np.uint64)) if len(ia) else 0
    return (na, nb, len(ia), int(ca.astype(np.uint64).sum(dtype=np.uint64)), int(cb.astype(np.uint64).sum(dtype=np.uint64)), smin)


def compare(sketches, pairs):
    """uint64 [n_pairs, 6] in the order of FIELDS."""
    out = np.zeros((len(pairs), 6), np.uint64)
    memo = {}
    for p, (i, j) in enumerate(pairs):
        if (i, j) not in memo:
            memo[(i, j)] = compare_pair(sketches[i], sketches[j])
        out[p] = memo[(i, j)]
    return out


def all_pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def pair_scaled(a, b):
    """The `scaled` a pair is compared at: the coarser one."""
    return a[3] if max_hash(a[3]) <= max_hash(b[3]) else b[3]


def ratio(num, den):
    return "NA" if den == 0 else "%.6f" % (num / den)


def table(names, sketches, pairs, records, ksize, min_jaccard=None):
    """The text `fingerprint-compare -o` writes."""
    lines = [f"##sketches={len(names)}", f"##pairs={len(pairs)}", f"##ksize={ksize}", HEADER]
    for (i, j), r in zip(pairs, records):
        na, nb, nc, sa, sb, sm = (int(x) for x in r)
        uni = na + nb - nc
        if min_jaccard is not None and (uni == 0 or nc / uni < min_jaccard):
            continue
        lines.append("\t".join([names[i], names[j], str(pair_scaled(sketches[i], sketches[j])), str(na), str(nb), str(nc), str(uni),
                                ratio(nc, uni), ratio(nc, na), ratio(nc, nb), str(sa), str(sb), str(sm), ratio(sm, sa + sb - sm)]))
    return "\n".join(lines) + "\n"


def matrix(names, sketches):
    """The text of `--matrix`."""
    n = len(names)
    lines = ["\t".join(["#name"] + list(names))]
    for i in range(n):
        row = [names[i]]
        for j in range(n):
            if i == j:
                row.append("1.000000" if len(sketches[i][0]) else "NA")
            else:
                na, nb, nc = compare_pair(sketches[i], sketches[j])[:3]
                row.append(ratio(nc, na + nb - nc))
        lines.append("\t".join(row))
    return "\n".join(lines) + "\n"
