"""The host side of phase-sites, without a device: dut_link_measure against the independent reference tests/link_ref.py on the
hand-derived golden case, the planted and the random inputs of tests/link_cases.py, in both forms; the pair set; the integer
rule that names a pair cis or trans; the sites file's parser; the TSV byte for byte; the CLI's argument checks; and the read
walk itself (csrc/link_walk.h) with dut_link_measure as a program of their own under AddressSanitizer + UBSan."""
import bisect
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import link_cases as S
import link_ref as R
import long_cases as LS
from decodingustools_amd import EngineError, LinkResult, build as _b, variants as V
from decodingustools_amd.callable_loci import DEL_CANDIDATE, SCAN_CANDIDATE, DelResult, ScanResult
from decodingustools_amd.records import ContigRecords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "link_kat.json")))


def measure(case, D, K, mq, flt, sites=None):
    ex, bq = (None, None) if flt is None else (flt[0], S.MBQ if flt[1] else None)
    return V.link_measure(case.rec, S.L, case.sites if sites is None else sites, D, K, mq, exclude_flags=ex, min_base_quality=bq)


def kat_records():
    return ContigRecords.from_reads([(r["pos"], r["cigar"], r["mapq"], 30, r["flag"], f"kat{i}", r["seq"]) for i, r in enumerate(KAT["reads"])])


def kat_counts():
    tables = np.zeros((len(KAT["tables"]), 6, 6), np.uint32)
    site_counts = np.zeros((len(KAT["sites"]), 6), np.uint32)
    for p, cells in enumerate(KAT["tables"]):
        for cell, n in cells.items():
            a, b = cell.split(",")
            tables[p, R.CLASSES.index(a), R.CLASSES.index(b)] = n
    for i, cells in enumerate(KAT["site_counts"]):
        for c, n in cells.items():
            site_counts[i, R.CLASSES.index(c)] = n
    return dict(first=np.array(KAT["first"], np.uint32), tables=tables, site_counts=site_counts)


def test_the_golden_case_by_the_reference_by_the_host_route_and_its_tsv(tmp_path):
    rec, want = kat_records(), kat_counts()
    args = (KAT["sites"], KAT["max_dist"], KAT["max_partners"], KAT["min_quality"])
    assert R.differences(R.counts(R.expand(rec), rec, KAT["contig_len"], *args, KAT["exclude_flags"]), want) == []
    got = V.link_measure(rec, KAT["contig_len"], *args, exclude_flags=KAT["exclude_flags"])
    assert R.differences(got, want) == []
    text = "\n".join(KAT["tsv"]) + "\n"
    out = str(tmp_path / "o.tsv")
    kw = dict(max_dist=KAT["max_dist"], max_partners=KAT["max_partners"], min_depth=KAT["min_depth"], min_quality=KAT["min_quality"],
              min_link_count=KAT["min_link_count"], exclude_flags=KAT["exclude_flags"])
    V.write_links(out, KAT["contig"], KAT["sites"], got, max_discordance=KAT["max_discordance"], **kw)
    assert open(out).read() == text
    # the reference writes the same bytes, so the device tests may hold the tool against it
    assert R.expected_tsv(KAT["contig"], KAT["sites"], want, max_discord_per_10k=500, **kw) == text


def test_the_reference_and_the_host_route_give_what_the_pinned_reads_say_by_themselves():
    for name, read, sites, flt, mq, seen in S.PINS:
        rec = ContigRecords.from_reads([read])
        exp = S.pin_expected(sites, seen)
        ex, bq = (None, None) if flt is None else (flt[0], S.MBQ if flt[1] else None)
        assert R.differences(R.counts(R.expand(rec), rec, S.L, sites, S.PIN_D, S.PIN_K, mq, ex, bq), exp) == [], name
        assert R.differences(V.link_measure(rec, S.L, sites, S.PIN_D, S.PIN_K, mq, exclude_flags=ex, min_base_quality=bq), exp) == [], name
    assert len(S.PINS) >= 20
    # what the planted reads were planted for shows in the reference's own tables
    c = S.planted()
    z = c.expected(S.PIN_D, S.PIN_K, 20, (0x704, False))
    sites = [int(s) for s in c.sites]
    i = sites.index(S.DEEP[0])
    deep = z["tables"][int(z["first"][i])].astype(np.int64)
    assert int(z["first"][i + 1]) - int(z["first"][i]) == 1 and deep[0, 1] > 255 and deep.sum() > 512 and deep[R.DEL].sum() > 0 and deep[:, R.OTHER].sum() > 0
    k = sites.index(S.CLUSTER[0])
    assert int(z["first"][k + 1]) - int(z["first"][k]) == 15 and sites[k + 16] - sites[k] <= S.PIN_D
    for lonely in (S.LONELY, S.EMPTY):
        j = sites.index(lonely)
        assert int(z["first"][j + 1]) == int(z["first"][j])
    assert int(z["site_counts"][sites.index(S.LONELY)].sum()) > 10 and int(z["site_counts"][sites.index(S.EMPTY)].sum()) == 0
    assert c.expected(S.PIN_D, S.PIN_K, 0, None)["tables"].sum() > c.expected(S.PIN_D, S.PIN_K, 20, None)["tables"].sum() > z["tables"].sum()
    assert c.expected(S.PIN_D, S.PIN_K, 20, (0x704, True))["tables"].sum() < z["tables"].sum()


@pytest.mark.parametrize("which", ["planted", "random-1", "random-2", "random-3"])
def test_host_route_equals_the_reference(which):
    case, (D, K) = {name: (c, dk) for name, c, dk in S.all_cases()}[which]
    if which != "planted":
        assert S.hollow(case, D, K) is None
    for mq, flt in itertools.product(S.QUALS, S.FILTERS):
        assert R.differences(measure(case, D, K, mq, flt), case.expected(D, K, mq, flt)) == [], (which, mq, flt)
    # other pair sets over the same sites; a pair's table does not depend on the set it is in
    whole = case.expected(D, K, 20, (0x704, True))
    for d, k in ((1, 1), (7, 2), (1000, 4)):
        want = case.expected(d, k, 20, (0x704, True))
        assert R.differences(measure(case, d, k, 20, (0x704, True)), want) == [], (which, d, k)
        if d <= D and k <= K:
            for i in range(len(case.sites)):
                n = int(want["first"][i + 1]) - int(want["first"][i])
                assert np.array_equal(want["tables"][int(want["first"][i]):int(want["first"][i]) + n], whole["tables"][int(whole["first"][i]):int(whole["first"][i]) + n])
    # a tile in descending coordinate order and a shuffled one: the same counts
    for order in (sorted(case.reads, key=lambda r: -r[0]), S.random.Random(3).sample(case.reads, len(case.reads))):
        other = S.Case(order, case.sites, sort=False)
        assert R.differences(measure(other, D, K, 20, (0x704, True)), whole) == []
    # no sites, one site
    none = measure(case, D, K, 20, None, sites=[])
    assert none.first.tolist() == [0] and none.tables.shape == (0, 6, 6) and none.site_counts.shape == (0, 6)
    one = measure(case, D, K, 20, None, sites=case.sites[5:6])
    assert one.first.tolist() == [0, 0] and np.array_equal(one.site_counts[0], case.expected(D, K, 20, None)["site_counts"][5])


def test_host_route_equals_the_reference_on_long_reads():
    """The tile of tests/long_cases.py: pairs further apart than 65 535 positions inside one read, reads past 65 535 stored
    bases and past 65 535 operations, a read over a 50 000N."""
    case = LS.whole()
    LS.check_shape(case)
    far = 0
    sites = np.array(LS.SITES, np.int64)
    for (D, K), mq, flt in ((pairs, mq, flt) for pairs in LS.LINK_SETS for mq, flt in LS.LINK_COMBOS[pairs]):
        ex, bq = (None, None) if flt is None else (flt[0], LS.MBQ if flt[1] else None)
        want = case.link_expected(D, K, mq, flt)
        assert R.differences(V.link_measure(case.rec, LS.LC, LS.SITES, D, K, mq, exclude_flags=ex, min_base_quality=bq), want) == [], (D, K, mq, flt)
        first = want["first"].astype(np.int64)
        anchor = np.repeat(np.arange(len(sites)), np.diff(first))
        partner = anchor + 1 + np.arange(int(first[-1])) - first[anchor]
        far = max(far, int(((sites[partner] - sites[anchor] > 65_535) & (want["tables"].sum((1, 2)) > 0)).sum()))
    assert far >= 20
    # a tile in descending coordinate order and a shuffled one: the same counts
    for order in (sorted(case.reads, key=lambda r: -r[0]), S.random.Random(3).sample(case.reads, len(case.reads))):
        other = LS.Case(order, sort=False)
        assert R.differences(V.link_measure(other.rec, LS.LC, LS.SITES, 70_000, 15, 0, exclude_flags=0x704, min_base_quality=LS.MBQ),
                             case.link_expected(70_000, 15, 0, (0x704, True))) == []


def test_host_route_with_one_thread_and_with_four():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import link_cases as S, link_ref as R, test_link_host as T\n"
            "for name, case, (D, K) in S.all_cases()[:2]:\n"
            "    for mq, flt in ((20, None), (0, (0x704, True))):\n"
            "        assert R.differences(T.measure(case, D, K, mq, flt), case.expected(D, K, mq, flt)) == [], (name, mq, flt)\n"
            "print('same')\n") % (ROOT, os.path.join(ROOT, "tests"))
    for threads in ("1", "4"):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, DUT_THREADS=threads))
        assert r.returncode == 0 and r.stdout.strip() == "same", (threads, r.stderr[-2000:])


def test_the_pair_set():
    # a 16th site within max_dist is not a partner
    sites = list(range(100, 100 + 17))
    assert V.link_pair_offsets(sites, 1000, 15)[:3].tolist() == [0, 15, 30] and int(V.link_pair_offsets(sites, 1000, 15)[-1]) == sum(min(15, 16 - i) for i in range(17))
    # distance exactly max_dist is a partner, one more is not; the last site has none
    assert V.link_pair_offsets([10, 60, 61], 50, 4).tolist() == [0, 1, 2, 2]
    assert V.link_pair_offsets([10, 61, 62], 50, 4).tolist() == [0, 0, 1, 1]
    assert V.link_pair_offsets([10, 60, 110], 50, 4).tolist() == [0, 1, 2, 2]
    assert V.link_pair_offsets([10, 11, 12, 13], 1000, 1).tolist() == [0, 1, 2, 3, 3]
    assert V.link_pair_offsets([], 5, 5).tolist() == [0] and V.link_pair_offsets([7], 5, 5).tolist() == [0, 0]
    # a site far behind a near one: the walk over the partners stops at the first that is too far
    assert V.link_pair_offsets([0, 5, 2 ** 32 - 1], 10, 15).tolist() == [0, 1, 1, 1]
    rng = S.random.Random(9)
    for _ in range(50):
        sites = sorted(rng.sample(range(3000), rng.randint(0, 60)))
        d, k = rng.randint(1, 300), rng.randint(1, 15)
        assert np.array_equal(V.link_pair_offsets(sites, d, k), R.pair_set(sites, d, k)), (sites, d, k)
    for bad in (([3, 3], 5, 5), ([4, 3], 5, 5), ([1, 2], 0, 5), ([1, 2], 5, 0), ([1, 2], 5, 16)):
        with pytest.raises(EngineError):
            V.link_pair_offsets(*bad)
    # the host route refuses what the engine refuses
    c = S.planted()
    for sites, d, k in (([5, 5], 10, 4), ([9, 5], 10, 4), ([5], 0, 4), ([5], 10, 0), ([5], 10, 16), ([S.L], 10, 4)):
        with pytest.raises(EngineError):
            V.link_measure(c.rec, S.L, sites, d, k, 20)


def table(**cells):
    t = np.zeros((6, 6), np.uint32)
    for k, n in cells.items():
        t[R.CLASSES.index(k[0] if k[0] != "d" else "del"), R.CLASSES.index(k[1] if k[1] != "d" else "del")] = n
    return t


def test_summarise_every_class_and_the_tie_rules():
    a, b = [80, 20, 0, 0, 0, 3], [0, 0, 75, 25, 0, 0]                             # major A minor C; major G minor T
    cis = table(AG=75, CT=20, AT=0, CG=0)
    u = V.link_summarise(a, b, cis, 10, 3, 500)
    assert (u["status"], u["major_a"], u["minor_a"], u["major_b"], u["minor_b"]) == (V.LINK_CIS, 0, 1, 2, 3)
    assert (u["MM"], u["Mm"], u["mM"], u["mm"], u["both"], u["other"], u["depth_a"], u["depth_b"]) == (75, 0, 0, 20, 95, 0, 103, 100)
    # one discordant read in 21 with a minor allele: 10000 * 1 <= 500 * 21; two in 22 are too many (20000 > 11000)
    assert V.link_summarise(a, b, table(AG=75, CT=20, AT=1), 10, 3, 500)["status"] == V.LINK_CIS
    assert V.link_summarise(a, b, table(AG=75, CT=20, AT=1, CG=1), 10, 3, 500)["status"] == V.LINK_UNRESOLVED
    assert V.link_summarise(a, b, table(AG=75, CT=20, AT=1, CG=1), 10, 3, 1000)["status"] == V.LINK_CIS
    trans = table(AG=60, AT=20, CG=15)
    assert V.link_summarise(a, b, trans, 10, 3, 500)["status"] == V.LINK_TRANS
    assert V.link_summarise(a, b, table(AG=60, AT=20, CG=15, CT=2), 10, 3, 500)["status"] == V.LINK_UNRESOLVED      # 20000 > 500 * 37
    assert V.link_summarise(a, b, table(AG=60, AT=20, CG=2), 10, 3, 500)["status"] == V.LINK_UNRESOLVED             # mM below min_link_count
    assert V.link_summarise(a, b, table(AG=60, CT=2), 10, 3, 500)["status"] == V.LINK_UNRESOLVED                    # mm below min_link_count
    assert V.link_summarise(a, b, table(AG=60), 10, 3, 500)["status"] == V.LINK_UNRESOLVED                          # m = 0
    # low_depth comes first and looks at the four cells only: nine reads there, whatever lies elsewhere
    u = V.link_summarise(a, b, table(AG=3, CT=6, Ad=40, dG=7), 10, 3, 500)
    assert (u["status"], u["both"], u["other"]) == (V.LINK_LOW_DEPTH, 56, 47)
    assert V.link_summarise(a, b, table(AG=4, CT=6, Ad=40), 10, 3, 500)["status"] == V.LINK_CIS
    # ties: the first of A C G T del wins as major, the first of the rest as minor; `other` is never an allele; del can be one
    u = V.link_summarise([5, 5, 5, 0, 5, 9], [0, 0, 0, 0, 0, 0], table(), 1, 1, 0)
    assert (u["major_a"], u["minor_a"], u["major_b"], u["minor_b"], u["status"]) == (0, 1, 0, 1, V.LINK_LOW_DEPTH)
    u = V.link_summarise([0, 0, 0, 2, 7, 50], [1, 0, 0, 0, 1, 0], table(dA=5, Td=2), 1, 1, 0)
    assert (u["major_a"], u["minor_a"], u["major_b"], u["minor_b"]) == (4, 3, 0, 4) and (u["MM"], u["mm"], u["status"]) == (5, 2, V.LINK_CIS)
    # refusals
    for kw in (dict(min_depth=0), dict(min_link_count=0), dict(max_discord_per_10k=5000)):
        with pytest.raises(EngineError):
            V.link_summarise(a, b, cis, **kw)
    with pytest.raises(ValueError):
        V.link_summarise(a[:5], b, cis)
    # the restatement the device tests build their TSV from says the same, on random counts
    rng = S.random.Random(4)
    for _ in range(300):
        ca, cb = [rng.choice((0, 1, 5, 5, 30)) for _ in range(6)], [rng.choice((0, 2, 2, 9)) for _ in range(6)]
        t = np.array([rng.choice((0, 0, 1, 3, 4, 40)) for _ in range(36)], np.uint32)
        prm = (rng.choice((1, 10, 50)), rng.choice((1, 3)), rng.choice((0, 1, 500, 2500, 4999)))
        assert V.link_summarise(ca, cb, t, *prm) == R.summarise(ca, cb, t, *prm), (ca, cb, t, prm)


def test_cis_and_trans_never_both_hold_and_products_are_taken_in_64_bits():
    # brute force over small counts: the two rules, each asked on its own, never both hold
    for d in (0, 1, 2500, 4999):
        for Mm, mM, mm in itertools.product(range(8), repeat=3):
            m = Mm + mM + mm
            for k in (1, 2, 3):
                cis = mm >= k and 10000 * (Mm + mM) <= d * m
                trans = Mm >= k and mM >= k and 10000 * mm <= d * m
                assert not (cis and trans), (d, Mm, mM, mm, k)
                u = V.link_summarise([9, 1, 0, 0, 0, 0], [9, 1, 0, 0, 0, 0], table(AA=1, AC=Mm, CA=mM, CC=mm), 1, k, d)
                assert u["status"] == (V.LINK_CIS if cis else V.LINK_TRANS if trans else V.LINK_UNRESOLVED), (d, Mm, mM, mm, k)
    # ... while at 5000 they could: the bound of the interval is what excludes it
    assert 1 >= 1 and 10000 * (1 + 1) <= 5000 * 4 and 10000 * 2 <= 5000 * 4
    # counts near 2^32: 10000 * count does not fit 32 bits
    big = 2 ** 32 - 1
    u = V.link_summarise([big, big - 1, 0, 0, 0, 0], [big, big - 1, 0, 0, 0, 0], table(AA=big, CC=big, AC=214748), 1, 1, 1)
    assert (u["status"], u["both"], u["mm"]) == (V.LINK_CIS, 2 * big + 214748, big)          # 10000 * 214748 <= 1 * (2^32 - 1 + 214748)
    assert V.link_summarise([big, big - 1, 0, 0, 0, 0], [big, big - 1, 0, 0, 0, 0], table(AA=big, CC=big, AC=429540), 1, 1, 1)["status"] == V.LINK_UNRESOLVED
    u = V.link_summarise([big, big - 1, 0, 0, 0, 0], [big, big - 1, 0, 0, 0, 0], table(AC=big, CA=big, CC=858993), 1, 1, 1)
    assert u["status"] == V.LINK_TRANS and u == R.summarise([big, big - 1, 0, 0, 0, 0], [big, big - 1, 0, 0, 0, 0], table(AC=big, CA=big, CC=858993), 1, 1, 1)
    assert V.link_summarise([big, big - 1, 0, 0, 0, 0], [big, big - 1, 0, 0, 0, 0], table(AC=big, CA=big, CC=859165), 1, 1, 1)["status"] == V.LINK_UNRESOLVED


def test_the_sites_parser_takes_the_projects_own_tsvs(tmp_path):
    def column2(path, contig):
        return sorted({int(l.split("\t")[1]) - 1 for l in open(path) if l.strip() and not l.startswith("#") and l.split("\t")[0] == contig})

    fv = str(tmp_path / "v.tsv")
    c = np.zeros(3, SCAN_CANDIDATE)
    for i, (pos, ref, alt, depth) in enumerate(((100, "A", "G", 20), (110, "T", "C", 18), (4000, "G", "T", 13))):
        c[i] = (pos, ord(ref), ord(alt), (0, 0), depth if alt == "A" else 0, depth if alt == "C" else 0, depth if alt == "G" else 0, depth if alt == "T" else 0, depth)
    V.write_variants(fv, "chrM", ScanResult(start=50, end=5000, low_depth=30, mixed=2, uncomparable=5, match=4910, variant=3, candidates=c), 10, 20)
    sites, skipped = V.link_sites_parse(fv, "chrM")
    assert sites.tolist() == column2(fv, "chrM") and len(sites) == 3 and skipped == 0 and sites.dtype == np.uint32
    fd = str(tmp_path / "d.tsv")
    d = np.zeros(3, DEL_CANDIDATE)
    for i, pos in enumerate((301, 302, 900)):
        d[i] = (pos, ord("A"), (0, 0, 0), 14, 20, 7, 7, 7, 7)
    V.write_deletions(fd, "chrM", DelResult(start=100, end=5000, low_depth=5, kept=4892, deleted=3, candidates=d), 10, 20, 3, 7000)
    sites, skipped = V.link_sites_parse(fd, "chrM")
    assert sites.tolist() == column2(fd, "chrM") and len(sites) == 2 and skipped == 0
    none, skipped = V.link_sites_parse(fd, "chrY")
    assert none.shape == (0,) and skipped == 2
    # duplicates merged, the result sorted, other contigs counted, comments, empty lines, CRLF and further columns ignored
    own = str(tmp_path / "s.tsv")
    open(own, "w").write("#contig\tpos\n\nchrM\t500\tx\ty\nchr1\t7\nchrM\t20\r\nchrM\t500\n# a comment\nchrY\t9\tz\nchrM\t4294967295\nchrM\t1")
    sites, skipped = V.link_sites_parse(own, "chrM")
    assert sites.tolist() == [0, 19, 499, 2 ** 32 - 2] and skipped == 2
    assert V.link_sites_parse(own, "chrX")[0].shape == (0,) and V.link_sites_parse(own, "chrX")[1] == 7
    # a malformed line is named by its number
    for text, line in (("chrM\t5\nchrM\n", 2), ("chrM\t5\n\n#c\nchrM\tfive\n", 4), ("chrM\t0\n", 1), ("chrM\t4294967296\n", 1), ("chrM\t-3\n", 1), ("\t5\n", 1),
                       ("chr1\t12\nchr1\t1.5\n", 2)):
        open(own, "w").write(text)
        with pytest.raises(EngineError) as e:
            V.link_sites_parse(own, "chrM")
        assert f"line {line}:" in str(e.value), (text, str(e.value))
    with pytest.raises(EngineError) as e:
        V.link_sites_parse(str(tmp_path / "absent.tsv"), "chrM")
    assert "absent.tsv" in str(e.value)


def test_the_writer_byte_for_byte(tmp_path):
    out = str(tmp_path / "o.tsv")
    sites = [9, 19, 59, 5000]
    first = V.link_pair_offsets(sites, 50, 4)
    assert first.tolist() == [0, 2, 3, 3, 3]
    sc = np.array([[80, 20, 0, 0, 0, 3], [0, 0, 75, 25, 0, 0], [0, 9, 0, 0, 9, 0], [0, 0, 0, 0, 0, 0]], np.uint32)
    tables = np.stack([table(AG=75, CT=20), table(AC=4, Ad=3, Cd=1), table(GC=30, Gd=12, TC=11)])
    res = LinkResult(first=first, tables=tables, site_counts=sc)
    V.write_links(out, "chrM", sites, res, sites_skipped=7, max_dist=50, max_partners=4, min_depth=10, min_quality=0, min_link_count=3, max_discordance="0.0125",
                  min_base_quality=13, exclude_flags=0x704)
    want = ("##contig=chrM\n##sites=4\n##sites_skipped=7\n##pairs=3\n##max_dist=50\n##max_partners=4\n##min_depth=10\n##min_quality=0\n"
            "##min_base_quality=13\n##exclude_flags=0x0704\n##min_link_count=3\n##max_discordance=0.0125\n"
            "##low_depth=1\n##cis=1\n##trans=1\n##unresolved=0\n"
            "#contig\tpos_a\tpos_b\tdist\tmajor_a\tminor_a\tmajor_b\tminor_b\tdepth_a\tdepth_b\tboth\tMM\tMm\tmM\tmm\tother\tstatus\n"
            "chrM\t10\t20\t10\tA\tC\tG\tT\t103\t100\t95\t75\t0\t0\t20\t0\tcis\n"
            "chrM\t10\t60\t50\tA\tC\tC\tdel\t103\t18\t8\t4\t3\t0\t1\t0\tlow_depth\n"
            "chrM\t20\t60\t40\tG\tT\tC\tdel\t100\t18\t53\t30\t12\t11\t0\t0\ttrans\n")
    assert open(out).read() == want
    assert R.expected_tsv("chrM", sites, dict(first=first, tables=tables, site_counts=sc), 7, 50, 4, 10, 0, 3, 125, 13, 0x704) == want
    # no sites: the comment lines and the header
    V.write_links(out, "chrM", [], LinkResult(first=np.zeros(1, np.uint32), tables=np.zeros((0, 6, 6), np.uint32), site_counts=np.zeros((0, 6), np.uint32)))
    text = open(out).read()
    assert text == R.expected_tsv("chrM", [], dict(first=[0], tables=[], site_counts=[])) and "##min_base_quality=.\n##exclude_flags=0x0000\n" in text
    assert "##max_discordance=0.0500\n" in text and text.endswith("\tstatus\n")
    # a result of another pair set, refused options
    with pytest.raises(EngineError):
        V.write_links(out, "chrM", sites, res, max_dist=10, max_partners=4)
    with pytest.raises(ValueError):
        V.write_links(out, "chrM", sites[:3], res, max_dist=50)
    for kw in (dict(min_depth=0), dict(min_link_count=0), dict(max_dist=0), dict(max_partners=16)):
        with pytest.raises((EngineError, ValueError)):
            V.write_links(out, "chrM", sites, res, **dict(dict(max_dist=50), **kw))
    for text in ("0.5", "0.05001", "-0.1", "5%", ""):
        with pytest.raises(ValueError):
            V.write_links(out, "chrM", sites, res, max_dist=50, max_discordance=text)
    assert V.link_discordance_parse("0") == 0 and V.link_discordance_parse("0.4999") == 4999 and V.link_discordance_parse(".05") == 500
    with pytest.raises(EngineError):
        V.write_links(str(tmp_path / "no" / "such" / "dir.tsv"), "chrM", sites, res, max_dist=50)


def test_cli_argument_errors_exit_2_without_a_device(tmp_path):
    out = str(tmp_path / "o.tsv")
    base = [_b.CLI, "phase-sites", "absent.bam", "-r", "absent.fa", "-o", out]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")

    def run(*args):
        return subprocess.run(base + list(args), capture_output=True, text=True, env=env)

    ok = ["-L", "chrM", "--sites", "absent.tsv"]
    for args in (["--sites", "absent.tsv"],                                             # no -L
                 ["-L", "chrM"],                                                        # no --sites
                 ok + ["--max-dist", "0"], ok + ["--max-dist=far"],
                 ok + ["--max-partners", "0"], ok + ["--max-partners", "16"], ok + ["--max-partners=x"],
                 ok + ["--min-depth", "0"], ok + ["--min-link-count", "0"],
                 ok + ["--max-discordance", "0.5"], ok + ["--max-discordance", "0.05001"], ok + ["--max-discordance", "5%"], ok + ["--max-discordance=-0.1"],
                 ok + ["--min-base-quality", "256"], ok + ["--min-base-quality", "q"],
                 ok + ["--exclude-flags", "0x"], ok + ["--exclude-flags", "70000"],
                 ok + ["--min-quality", "300"], ok + ["--region", "5-9"], ok + ["--no-such-flag"]):
        r = run(*args)
        assert r.returncode == 2 and r.stderr and not os.path.exists(out), (args, r.returncode, r.stderr[-300:])
    r = subprocess.run([_b.CLI, "phase-sites", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "phase-sites" in r.stderr and "--max-partners" in r.stderr
    # the files are looked at only behind the arguments: an unreadable sites file is exit 1 and names it; so is a malformed one
    r = run(*ok, "--max-partners", "15", "--max-discordance", "0.4999", "--max-dist", "1")
    assert r.returncode == 1 and "absent.tsv" in r.stderr
    bad = str(tmp_path / "bad.tsv")
    open(bad, "w").write("chrM\t12\nchrM\ttwelve\n")
    r = run("-L", "chrM", "--sites", bad)
    assert r.returncode == 1 and "line 2" in r.stderr


def fnv(words, h=14695981039346656037):
    for w in words:
        for k in range(4):
            h = ((h ^ ((int(w) >> (8 * k)) & 255)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_walk_and_host_route_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "link_walk_host")
    # (variants.cpp alone: what its file-level functions call of the engine and the readers stays unresolved -- this program
    # calls none of them)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "link_walk_host.cpp"), os.path.join(ROOT, "decodingustools_amd", "csrc", "variants.cpp"),
           "-Wl,--unresolved-symbols=ignore-all", "-lpthread", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if any(m in r.stderr for m in ("cannot find -lasan", "cannot find -lubsan", "unrecognized command-line option", "unrecognized argument")):
            pytest.skip("sanitizer runtimes not installed here: " + r.stderr[-300:])
        pytest.fail("the sanitizer build failed:\n" + r.stderr[-3000:])
    # max_dist max_partners min_quality filtered exclude_flags has_min_base_quality min_base_quality
    short = [(1000, 15, 20, 1, 0x704, 1, S.MBQ), (1000, 15, 0, 0, 0, 0, 0), (1, 1, 20, 1, 0, 0, 0), (40, 4, 0, 1, 0xFFFF, 1, S.MBQ), (2 ** 32 - 1, 15, 20, 1, 0, 1, S.MBQ)]
    # the long reads: the walk's pair set reaches 70 000 positions, fifteen partners
    long = [(70_000, 15, 20, 1, 0x704, 1, LS.MBQ), (2 ** 32 - 1, 15, 0, 0, 0, 0, 0), (1, 1, 20, 1, 0, 0, 0), (1000, 4, 0, 1, 0xFFFF, 1, LS.MBQ)]
    for name, case, L, configs in (("planted", S.planted(), S.L, short), ("random", S.randomised(1), S.L, short), ("long", LS.whole().as_link, LS.LC, long)):
        rec, ev = case.rec, case.events
        sites = [int(s) for s in case.sites]
        lines = [f"{L} {rec.n} {len(sites)} {len(configs)}"] + LS.read_lines(rec)
        lines.append(" ".join(str(s) for s in sites))
        lines += [" ".join(str(x) for x in c) for c in configs]
        path = str(tmp_path / f"{name}.txt")
        open(path, "w").write("\n".join(lines) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=0", DUT_THREADS="3"))
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
        # the walk: per read and covered anchor the 16 observations under the first configuration, from the reference's maps
        D, K, thr = configs[0][0], configs[0][1], configs[0][6]
        first = R.pair_set(sites, D, K)
        words = []
        for rr in range(rec.n):
            lo, hi = int(ev["lo"][rr]), int(ev["hi"][rr])
            if not (0 <= lo < L) or hi <= lo:
                continue
            for i in range(bisect.bisect_left(sites, lo), bisect.bisect_left(sites, hi)):
                packed = 0
                for k in range(16):
                    o = ev["maps"][rr].get(sites[i + k]) if k <= int(first[i + 1]) - int(first[i]) else None
                    packed |= (15 if o is None or o[1] < thr else o[0]) << (4 * k)
                words += [packed & 0xFFFFFFFF, packed >> 32]
        want = [f"walk {fnv(words):016x}"]
        for k, (D, K, mq, filtered, ex, has_bq, bq) in enumerate(configs):
            z = R.counts(ev, rec, L, sites, D, K, mq, ex if filtered else None, bq if has_bq else None)
            want.append(f"measure {k} {fnv(list(z['first']) + list(z['tables'].reshape(-1)) + list(z['site_counts'].reshape(-1))):016x}")
        assert r.stdout.splitlines() == want, (name, r.stdout, want)
