"""A pure-Python model of the runlist JSON loaders (gams_amd/csrc/runlist.hip, gams_amd/host/gams_runlist.cpp) and the
documents their tests share: the JSON structure check, the device grammar and the host grammar as two predicates,
IntSpan normalisation, and build_dir over a group's spans (the arithmetic of tests/interval_edges.py).

`intspan` is off-tree: beyond the intergenic.json fixture this grammar is parity unpinned.  Nothing here
imports the GPU package.
"""
import json
import re

import numpy as np

import interval_edges as ie

I32_MIN, I32_MAX = -2**31, 2**31 - 1


class Invalid(ValueError):
    """where the host reader answers GAMS_EINVAL (the reference panics)"""


class _Pairs(list):
    pass


# ---- the JSON structure check ----------------------------------------------------------------------------------------
def json_pairs(data):
    """(key, value string) of a flat JSON object of string values, in file order; Invalid otherwise"""
    try:
        text = bytes(data).decode("utf-8")
        doc = json.loads(text, object_pairs_hook=_Pairs)
    except (ValueError, RecursionError) as e:          # UnicodeDecodeError and JSONDecodeError are ValueErrors
        raise Invalid(str(e))
    if not isinstance(doc, _Pairs):
        raise Invalid("not an object")
    for k, v in doc:
        if not isinstance(v, str) or isinstance(v, _Pairs):
            raise Invalid("a value that is not a string")
        if any(0xD800 <= ord(c) <= 0xDFFF for c in k + v):
            raise Invalid("a lone surrogate")
    return list(doc)


# ---- the two grammars of one runlist ---------------------------------------------------------------------------------
_HOST_TOKEN = re.compile(r"^(-?[0-9]+)(?:-(-?[0-9]+))?$")
_DEV_TOKEN = re.compile(r"^([0-9]{1,10})(?:-([0-9]{1,10}))?$")


def host_spans(value):
    """the raw spans of a runlist as the host reader takes it: negative numbers, empty tokens skipped; Invalid otherwise"""
    if re.search(r"[^0-9,\-]", value):
        raise Invalid("a runlist character that is no digit, '-' or ','")
    if value in ("", "-"):
        return []
    out = []
    for tok in value.split(","):
        if tok == "":
            continue
        m = _HOST_TOKEN.match(tok)
        if not m:
            raise Invalid("a token that is not a or a-b")
        a = int(m.group(1))
        b = int(m.group(2)) if m.group(2) is not None else a
        if not (I32_MIN <= a <= I32_MAX and I32_MIN <= b <= I32_MAX):
            raise Invalid("a number outside i32")
        if a > b:
            raise Invalid("a > b")
        out.append((a, b))
    return out


def device_takes_value(value):
    """the device's grammar of one value: "" and "-" are the empty set, else tokens a or a-b of 1-10 digits, a <= b <= INT32_MAX"""
    if value in ("", "-"):
        return True
    for tok in value.split(","):
        m = _DEV_TOKEN.match(tok)
        if not m:
            return False
        a = int(m.group(1))
        b = int(m.group(2)) if m.group(2) is not None else a
        if a > b or b > I32_MAX:
            return False
    return True


_WS = r"[ \t\n\r]*"
_KEY = r'"[^"\x00-\x1f]*"'
_PAIR = _KEY + _WS + ":" + _WS + r'"[^"]*"'
_DEV_DOC = re.compile(r"^" + _WS + r"\{" + _WS + r"(?:" + _PAIR + r"(?:" + _WS + "," + _WS + _PAIR + r")*)?" + _WS + r"\}" + _WS + r"$")


def device_takes(data):
    """True where gams_spans_create_runlist_text builds the set, False where it answers GAMS_EUNSUPPORTED"""
    data = bytes(data)
    if any(b >= 0x80 or b == 0 or b == 0x5C for b in data):
        return False
    text = data.decode("ascii")
    if not _DEV_DOC.match(text):
        return False
    strings = re.findall(r'"([^"]*)"', text)
    keys, values = strings[0::2], strings[1::2]
    return len(set(keys)) == len(keys) and all(device_takes_value(v) for v in values)


# ---- IntSpan normalisation -------------------------------------------------------------------------------------------
def normalise(spans):
    """IntSpan::add_runlist: the union of the spans, overlapping and adjacent ones joined: (lo, hi) int32 arrays"""
    lo, hi = [], []
    for a, b in sorted(spans):
        if lo and a <= hi[-1] + 1:
            hi[-1] = max(hi[-1], b)
        else:
            lo.append(a)
            hi.append(b)
    return np.array(lo, np.int32), np.array(hi, np.int32)


def model(data):
    """{chr: (lo, hi)} of a runlist JSON file as the host reader gives it (a key that comes twice keeps its first place
    and its last value); Invalid where it answers GAMS_EINVAL"""
    out = {}
    for k, v in json_pairs(data):
        out[k] = normalise(host_spans(v))
    return out


def verdict(data):
    try:
        return model(data)
    except Invalid:
        return None


def same_sets(got, want):
    """two {chr: (lo, hi)}: the same keys in the same order and the same spans"""
    return list(got) == list(want) and all(np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1])
                                           for k in want)


def as_arrays(sets):
    """(group_off, lo, hi) of a {chr: (lo, hi)} for gams_spans_create"""
    off = np.cumsum([0] + [v[0].size for v in sets.values()]).astype(np.uint64)
    lo = np.concatenate([v[0] for v in sets.values()] + [np.zeros(0, np.int32)]).astype(np.int32)
    hi = np.concatenate([v[1] for v in sets.values()] + [np.zeros(0, np.int32)]).astype(np.int32)
    return off, lo, hi


# ---- build_dir over one group's spans --------------------------------------------------------------------------------
def span_dir(lo):
    """(key0, shift, nb, dir[nb + 1]) of build_dir over the biased lows of one group (gams_spans_create)"""
    if len(lo) == 0:
        return 0, 0, 0, np.zeros(1, np.uint32)
    key = np.asarray(lo, np.int64) + 2**31
    key0, shift, nb = ie.span_grid(lo)
    edges = key0 + (np.arange(nb, dtype=np.int64) << shift)
    d = np.searchsorted(key, edges, side="left").astype(np.uint32)
    return key0, shift, nb, np.append(d, np.uint32(key.size))


# ---- documents -------------------------------------------------------------------------------------------------------
def runlist_of(spans):
    """IntSpan::runlist of (lo, hi) pairs as given (no normalisation): a single position prints as one number"""
    return ",".join(str(a) if a == b else f"{a}-{b}" for a, b in spans)


def doc(pairs, pretty=False, crlf=False):
    """the JSON text of (key, runlist string) pairs with plain-ASCII keys, compact or as serde_json's to_string_pretty"""
    if pretty:
        nl = "\r\n" if crlf else "\n"
        body = ("," + nl).join(f'  "{k}": "{v}"' for k, v in pairs)
        return ("{" + nl + body + nl + "}" + nl if pairs else "{}" + nl).encode()
    return ("{" + ",".join(f'"{k}":"{v}"' for k, v in pairs) + "}").encode()


# name -> bytes: what the host reader accepts ...
EDGE_OK = {
    "escapes in keys": b'{"a\\"b\\\\c\\/\\b\\f\\n\\r\\t\\u0041\\u00e9\\ud83d\\ude00": "1-5", "x\\u0000y": "7"}',
    "utf-8 key": '{"chré中\U0001f600": "1-5"}'.encode(),
    "duplicate key": b'{"I": "1-5", "II": "7-9", "I": "20-30,40"}',
    "empty values": b'{"I": "", "II": "-", "III": "4"}',
    "negative spans": b'{"I": "-5--1,3-4,-20--10,-9"}',
    "empty tokens": b'{"I": ",1-2,,5,", "II": ","}',
    "joins into one": b'{"I": "30-40,1-10,11-20,15-35,41,42-50"}',
    "single number": b'{"I": "7"}',
    "int32 max": b'{"I": "2147483647", "II": "2147483646-2147483647,1", "III": "-2147483648--2147483647"}',
    "leading zeros": b'{"I": "007-0000000000010"}',
    "no group": b"{}",
    "no group, white space": b" \t\r\n{ \n } \n",
    "compact": doc([("I", "1-5,9"), ("II", "3")]),
    "pretty": doc([("I", "1-5,9"), ("II", "3")], pretty=True),
    "crlf": doc([("I", "1-5,9"), ("II", "3")], pretty=True, crlf=True),
    "empty key": b'{"": "1"}',
    "escape in value": b'{"I": "1\\u002d5"}',
}
# ... and what it answers GAMS_EINVAL to, each by its own document
EDGE_EINVAL = {
    "not an object: array": b'["1-5"]',
    "not an object: string": b'"1-5"',
    "not an object: empty": b"",
    "not an object: null": b"null",
    "non-string value: number": b'{"I": 5}',
    "non-string value: null": b'{"I": null}',
    "non-string value: nested": b'{"I": {"a": "1"}}',
    "non-string value: array": b'{"I": ["1-5"]}',
    "bad character: space": b'{"I": "1-5, 7"}',
    "bad character: letter": b'{"I": "1-5,x"}',
    "bad character: plus": b'{"I": "+5"}',
    "a > b": b'{"I": "5-3"}',
    "a > b negative": b'{"I": "-1--5"}',
    "outside i32": b'{"I": "2147483648"}',
    "outside i32 negative": b'{"I": "-2147483649-5"}',
    "outside i32 long": b'{"I": "99999999999999999999999"}',
    "dangling dash": b'{"I": "5-"}',
    "double dash": b'{"I": "--5"}',
    "lone dash token": b'{"I": "1,-"}',
    "three numbers": b'{"I": "1-2-3"}',
    "missing brace": b'{"I": "1-5"',
    "text behind the object": b'{"I": "1-5"} x',
    "trailing comma": b'{"I": "1-5",}',
    "missing colon": b'{"I" "1-5"}',
    "control character in key": b'{"I\n": "1-5"}',
    "bad escape": b'{"I\\x": "1-5"}',
    "lone surrogate": b'{"I\\ud800": "1-5"}',
    "invalid utf-8": b'{"I\xff": "1-5"}',
    "overlong utf-8": b'{"I\xc0\x80": "1-5"}',
    "byte order mark": b'\xef\xbb\xbf{"I": "1-5"}',
}


def seam_doc():
    """About 40 KiB, 6 groups: one without a span, one with one span, one whose value is longer than 16 KiB; 10-digit
    numbers throughout the long values so that quotes, commas, dashes and 10-digit numbers meet every boundary once
    the document is pushed along by a prefix of spaces"""
    rng = np.random.default_rng(20261020)

    def spans(n, base, step):
        lo = base + np.cumsum(rng.integers(2, step, n)) * 3
        ln = rng.integers(0, 3, n)
        return [(int(a), int(a + b)) for a, b in zip(lo, ln)]

    big = spans(1000, 1_000_000_000, 300)              # 10-digit numbers: about 20 KiB of text
    assert big[-1][1] <= I32_MAX
    pairs = [("I", runlist_of(spans(300, 0, 50))), ("none", ""), ("II", runlist_of(big)), ("one", "2147483647"),
             ("dash", "-"), ("III", runlist_of(spans(900, 999_999_000, 40)))]
    data = doc(pairs, pretty=True)
    assert 36 * 1024 < len(data) < 48 * 1024 and len(pairs[2][1]) > 16 * 1024
    return data


SEAM_PREFIXES = list(range(64)) + [4095, 4096, 4097, 16383, 16384, 16385]
