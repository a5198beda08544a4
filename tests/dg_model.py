"""A strict-f32 numpy model of the reference's DeltaG (src/libs/delta_g.rs), written from that file and not from the
library: the table of a (temp, salt) pair (init_delta_g, :118-207) and DeltaG::polymer (:78-115), every step one f32
operation in the reference's order.  Also the model of the `sw` text with the ΔG column, and the battery the CPU and GPU
tests share."""
import numpy as np

f32 = np.float32
BASES = b"ACGT"
# SantaLucia 1998 (delta_g.rs:120-171): dimer -> (dH kcal/mol, dS cal/K.mol)
NN = {"AA": (-7.6, -21.3), "TT": (-7.6, -21.3), "AT": (-7.2, -20.4), "TA": (-7.2, -21.3), "CA": (-8.5, -22.7),
      "TG": (-8.5, -22.7), "GT": (-8.4, -22.4), "AC": (-8.4, -22.4), "CT": (-7.8, -21.0), "AG": (-7.8, -21.0),
      "GA": (-8.2, -22.2), "TC": (-8.2, -22.2), "CG": (-10.6, -27.2), "GC": (-9.8, -24.4), "GG": (-8.0, -19.9),
      "CC": (-8.0, -19.9)}
KNOWN = [(37.0, 1.0, "TAACAAGCAATGAGATAGAGAAAGAAATATATCCA", -39.2702), (30.0, 0.1, "TAACAAGCAATGAGATAGAGAAAGAAATATATCCA", -35.6605),
         (37.0, 1.0, "GAATTC", -1.1399), (37.0, 1.0, "NAATTC", None)]          # delta_g.rs:209-234, within 0.001


def table(temp=37.0, salt=1.0):
    """21 f32: nn[4 * c(X) + c(Y)] with A C G T = 0 1 2 3, init[4], sym"""
    t = np.zeros(21, f32)
    adj = f32(0.368) * np.log(f32(salt)).astype(f32)
    for i, x in enumerate("ACGT"):
        for j, y in enumerate("ACGT"):
            dh, ds0 = NN[x + y]
            ds = f32(ds0) + adj
            t[4 * i + j] = f32(dh) - ((f32(273.15) + f32(temp)) * (ds / f32(1000.0)))
    t[16:20] = [0.05, 1.96, 1.96, 0.05]
    t[20] = 0.43
    return t


_CODE = np.full(256, 4, np.uint8)
for _i, _b in enumerate(BASES):
    _CODE[_b] = _CODE[_b | 0x20] = _i


def codes(seq):
    return _CODE[np.frombuffer(bytes(seq), np.uint8)]


def polymer(t, seq, tree=False):
    """the f32 of DeltaG::polymer, NaN for None.  tree=True sums the dimer terms pairwise (numpy's sum) instead of in
    sequence order: the model the battery must tell apart from the right one."""
    c = codes(seq)
    n = c.size
    if n < 3 or (c > 3).any():
        return f32(np.nan)
    terms = t[4 * c[:-1].astype(np.int64) + c[1:]]
    if tree:
        dg = np.sum(terms, dtype=f32)
    else:
        dg = f32(0.0)
        for x in terms:
            dg = f32(dg + x)
    dg = f32(dg + t[16 + c[0]])
    dg = f32(dg + t[16 + c[-1]])
    if n % 2 == 0 and np.all(c + c[::-1] == 3):
        dg = f32(dg + t[20])
    return dg


def fmt(v):
    """the tenth field: `{:.4}` of the f32, nothing for None"""
    return "" if np.isnan(v) else "%.4f" % float(f32(v))


def random_seq(rng, n, lower=0.2):
    s = np.frombuffer(BASES, np.uint8)[rng.integers(0, 4, n)]
    return np.where(rng.random(n) < lower, s | 0x20, s).astype(np.uint8).tobytes()


def battery(seed=1):
    """[(name, bytes)]: lengths 3..300 with 20 % lower case, one invalid byte first / last / in the middle, GAATTC,
    (AT)n for n = 2..60, even lengths that miss their reverse complement at the middle pair only, odd lengths"""
    rng = np.random.default_rng(seed)
    out = [(f"len{n}", random_seq(rng, n)) for n in range(3, 301)]
    for n in (3, 17, 100, 257):
        s = bytearray(random_seq(rng, n))
        for name, at in (("first", 0), ("last", n - 1), ("mid", n // 2)):
            b = bytearray(s)
            b[at] = rng.choice(np.frombuffer(b"N-nRY\x00\x80\xff@[`{", np.uint8))
            out.append((f"bad_{name}{n}", bytes(b)))
    out.append(("GAATTC", b"GAATTC"))
    out += [(f"AT{n}", b"AT" * n) for n in range(2, 61)]
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    for h in (2, 8, 33, 50):
        half = random_seq(rng, h)
        pal = half + half.translate(comp)[::-1]
        out.append((f"pal{2 * h}", pal))
        miss = bytearray(pal)
        miss[h] = ord("A") if pal[h] not in b"Aa" else ord("C")       # the middle pair alone
        out.append((f"pal_miss{2 * h}", bytes(miss)))
    out += [(f"odd{n}", random_seq(rng, n)) for n in (5, 99, 101, 299)]
    return out


def sw_text_with_dg(text, seq, chr_start, t):
    """rows of `gams sw` for one ctg (chr_start, its bases `seq`) -> the rows with the ΔG of each row's range column as
    a tenth field"""
    rows = []
    for row in text.splitlines():
        f = row.split("\t")
        rg = f[1].split(":")[1]
        s, _, e = rg.partition("-")
        s, e = int(s), int(e or s)
        rows.append(row + "\t" + fmt(polymer(t, seq[s - chr_start:e - chr_start + 1])))
    return "".join(r + "\n" for r in rows)
