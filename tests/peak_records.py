"""A pure-Python model of gams_gpu_peak_records_text / host.peak_records_text: the records `gams peak` stores
(peak.rs:68-78,163-171: SET peak:{ctg_id}:{serial} serde_json(Peak)) as TSV rows, "{id}\\t{json}\\n" rows or RESP SET
commands.  The eleven fields are those of tests/peak_text.py (oracle-backed), per ctg; the serial continues
serial_base; the JSON is data.rs:30-43 in serde's field order, without spaces: integers as printed, a float as its TSV
text with ".0" behind one without a point (serde_json's f32 is ryu's shortest round trip, always with a decimal point,
positional for 0 and [1e-5, 1]), strings escaped as serde_json escapes them."""
import peak_text as pt

KEYS = ["id", "range", "length", "gc", "signal", "left_wave_length", "left_amplitude", "left_signal",
        "right_wave_length", "right_amplitude", "right_signal"]
STRINGS = {"id", "range", "signal", "left_signal", "right_signal"}
FLOATS = {"gc", "left_amplitude", "right_amplitude"}
SHORT = {'"': '\\"', "\\": "\\\\", "\b": "\\b", "\t": "\\t", "\n": "\\n", "\f": "\\f", "\r": "\\r"}


def escape(s):
    """the contents of a JSON string as serde_json writes them"""
    return "".join(SHORT.get(ch) or ("\\u%04x" % ord(ch) if ord(ch) < 0x20 else ch) for ch in s)


def json_float(t):
    return t if "." in t else t + ".0"


def json_of(fields):
    """serde_json::to_string of the Peak whose TSV fields these are"""
    out = []
    for k, v in zip(KEYS, fields):
        if k in STRINGS:
            v = '"' + escape(v) + '"'
        elif k in FLOATS:
            v = json_float(v)
        out.append('"%s":%s' % (k, v))
    return "{" + ",".join(out) + "}"


def resp(*args):
    """wire::resp_command: an array of bulk strings, the lengths in bytes"""
    return "*%d\r\n" % len(args) + "".join("$%d\r\n%s\r\n" % (len(a), a) for a in args)


def record(fields, fmt):
    """one record from its eleven TSV fields (the id with its final serial)"""
    if fmt == "tsv":
        return "\t".join(fields) + "\n"
    if fmt == "resp":
        return resp("SET", fields[0], json_of(fields))
    assert fmt == "records"
    return fields[0] + "\t" + json_of(fields) + "\n"


def ctg_records(c, pk, fmt, base):
    """the records of one ctg from its sorted kept peaks, numbered behind base"""
    out = []
    for k, row in enumerate(pt.ctg_rows(c, pk).split("\n")[:-1]):
        f = row.split("\t")
        assert len(f) == 11 and f[0] == "peak:%s:%d" % (c["id"], k + 1)
        f[0] = "peak:%s:%d" % (c["id"], base + k + 1)
        out.append(record(f, fmt))
    return "".join(out)


def model(ctgs, data, fmt="records", serial_base=None):
    """-> (the text of host.peak_records_text(eng, ctgs, data, fmt, serial_base) as bytes, {ctg id: counter after})"""
    base = serial_base or {}
    _, kept = pt.buckets(ctgs, data)
    order = sorted(range(len(ctgs)), key=lambda i: ctgs[i]["id"].encode())
    text = "".join(ctg_records(ctgs[i], kept[i], fmt, base.get(ctgs[i]["id"], 0)) for i in order)
    return text.encode("latin-1"), {c["id"]: base.get(c["id"], 0) + len(kept[i]) for i, c in enumerate(ctgs)}
