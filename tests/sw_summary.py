"""A pure-Python model of the sw summary (host.sw_summary): the table of
templates/dql/fsw-distance.tera.sql and fsw-distance-tag.tera.sql over the TEXT of the sw rows.

It is fed the rows as text -- what tests/sw_text.py's model, ora.sw_proc_ctg or host.sw_text print, per file --, parses
every statistic as a decimal into the integer m of m / 10^4, groups with Python integers, rounds S / COUNT to the nearest
integer with ties to even in integer arithmetic and prints q / 10^4 with the trailing zeros dropped.  Nothing here comes
from the project's summariser."""

STATS = 4


def units(field):
    """a printed statistic as the integer m of m / 10^4; None for NaN.  "-0" is 0."""
    f = field.strip()
    if f in (b"NaN", b"nan"):
        return None
    neg = f.startswith(b"-")
    if neg:
        f = f[1:]
    ip, _, fr = f.partition(b".")
    assert ip.isdigit() and (fr == b"" or fr.isdigit()) and len(fr) <= 4, field
    m = int(ip) * 10000 + int((fr + b"0000")[:4])
    assert not (neg and m), field                      # the only negative a row prints is -0
    return m


class Table:
    """groups[(tag, distance)] = [COUNT, [S x 4], [NaN x 4], C]; tag None without tags"""

    def __init__(self, actions=("gc",)):
        self.gc, self.count = "gc" in actions, "count" in actions
        self.groups = {}

    def add_text(self, text, tag=None):
        """the rows of one file (bytes, no header)"""
        for row in text.split(b"\n"):
            if not row:
                continue
            f = row.split(b"\t")
            assert len(f) == 9, row
            g = self.groups.setdefault((tag, int(f[3])), [0, [0] * STATS, [0] * STATS, 0])
            g[0] += 1
            if self.gc:
                for k in range(STATS):
                    m = units(f[4 + k])
                    if m is None:
                        g[2][k] += 1
                    else:
                        g[1][k] += m
            if self.count:
                g[3] += int(f[8])
        return self

    def rows(self):
        return sum(g[0] for g in self.groups.values())

    def header(self, tagged):
        cols = (["tag"] if tagged else []) + ["distance"]
        if self.gc:
            cols += ["AVG_gc_content", "AVG_gc_mean", "AVG_gc_stddev", "AVG_gc_cv"]
        if self.count:
            cols += ["AVG_rg_count"]
        return "\t".join(cols + ["COUNT"]).encode() + b"\n"

    def text(self, tagged=False):
        out = [self.header(tagged)]
        for tag, d in sorted(self.groups, key=lambda k: (b"" if k[0] is None else k[0], k[1])):
            n, s, nan, c = self.groups[(tag, d)]
            f = ([tag] if tagged else []) + [b"%d" % d]
            if self.gc:
                f += [b"nan" if nan[k] else avg4(s[k], n) for k in range(STATS)]
            if self.count:
                f += [avg4(c * 10000, n)]
            out.append(b"\t".join(f + [b"%d" % n]) + b"\n")
        return b"".join(out)

    def arrays(self, mx, tags=None):
        """{(slot, distance): (COUNT, S, NaN, C)} laid out as host.sw_summary_table lays them out: lists indexed
        [slot][distance]"""
        slots = [None] if tags is None else sorted(set(tags))
        z = lambda: [[0] * (mx + 1) for _ in slots]
        z4 = lambda: [[[0] * STATS for _ in range(mx + 1)] for _ in slots]
        count, s, nan, c = z(), z4(), z4(), z()
        for (tag, d), g in self.groups.items():
            t = slots.index(tag)
            count[t][d], s[t][d], nan[t][d], c[t][d] = g[0], list(g[1]), list(g[2]), g[3]
        return dict(tags=None if tags is None else slots, count=count, sum=s, nan=nan, rg_count=c)


def round_half_even(num, den):
    q, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and q % 2 == 1):
        q += 1
    return q


def avg4(num, den):
    """num / den rounded to an integer q (ties to even), printed as q / 10^4 with the trailing zeros dropped"""
    q = round_half_even(num, den)
    ip, fr = divmod(q, 10000)
    s = b"%d" % ip
    if fr:
        s += b"." + (b"%04d" % fr).rstrip(b"0")
    return s


def ties(table):
    """[(tag, distance, column)] of the groups whose S / COUNT lies exactly between two integers"""
    return [(tag, d, k) for (tag, d), g in sorted(table.groups.items(), key=lambda kv: (kv[0][0] or b"", kv[0][1]))
            for k in range(STATS) if not g[2][k] and 2 * (g[1][k] % g[0]) == g[0]]


def tie_data(ctgs, rows_of, tries=64):
    """A feature file built to hold an exact tie: three point features in ctgs[0], of which the first is dropped, so the
    M group has COUNT 2; the first pair whose two gc_content m add up to an odd number is taken (rows_of(data) gives
    the rows' text).  -> the file's bytes"""
    c = ctgs[0]
    for k in range(tries):
        a, b = c["chr_start"] + 3000 + 53 * k, c["chr_start"] + 9000 + 31 * k
        data = ("%s:%d\n%s:%d\n%s:%d\n" % (c["chr_id"], c["chr_start"] + 500, c["chr_id"], a, c["chr_id"], b)).encode()
        g = Table().add_text(rows_of(data)).groups[(None, 0)]
        if g[0] == 2 and g[1][0] % 2 == 1:
            return data
    raise AssertionError("no tie in %d tries" % tries)


def summary(texts, tags=None, actions=("gc",)):
    """-> (the text of host.sw_summary, the Table) for the rows of several files, texts[f] under tags[f]"""
    t = Table(actions)
    for k, text in enumerate(texts):
        t.add_text(text, None if tags is None else tags[k])
    return t.text(tags is not None), t
