// gams_runlist.cpp -- the host reader of a runlist JSON file (anno.rs:84-87: intspan::read_json, then json2set): the
// complete reader, and the fallback behind gams_spans_create_runlist_text.  Plain C++17, no device call: the
// stand-alone driver tests/runlist_main.cpp links this unit alone.
//
// The file is one flat JSON object of string values.  Strings are read with their escapes (\" \\ \/ \b \f \n \r \t
// \uXXXX, surrogate pairs joined) and must be valid UTF-8 without control characters; any JSON white space may stand
// between the tokens; a key that comes twice keeps its first place and its last value.  GAMS_EINVAL covers where the
// reference panics: not an object, a value that is not a string (as_str().unwrap()), a runlist character that is no
// digit / '-' / ',', a > b, a number outside i32 -- and every malformed document.
//
// A runlist is tokens separated by ','; a token is `a` or `a-b`, each number an optional '-' and decimal digits
// (-5--1 is -5 .. -1); an empty token is skipped and the values "" and "-" are the empty set (IntSpan::add_runlist).
// The spans are normalised by sort and join: overlapping and adjacent ones become one.
#include <algorithm>
#include <numeric>

#include "gams_host.hpp"

namespace gams {
namespace {

struct JsonIn {
    const unsigned char *s;
    size_t n, p = 0;
    [[noreturn]] void fail(const std::string &what) const {
        throw Error(GAMS_EINVAL, "read_runlist_json: " + what + " at byte " + std::to_string(p));
    }
    void ws() {
        while (p < n && (s[p] == ' ' || s[p] == '\t' || s[p] == '\n' || s[p] == '\r')) ++p;
    }
    unsigned hex4() {
        if (n - p < 4) fail("a truncated \\u escape");
        unsigned v = 0;
        for (int k = 0; k < 4; ++k) {
            const unsigned char c = s[p++];
            const unsigned d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10u : c >= 'A' && c <= 'F' ? c - 'A' + 10u : 99u;
            if (d > 15u) fail("a \\u escape that is not four hex digits");
            v = v * 16u + d;
        }
        return v;
    }
    static void put_utf8(std::string &out, unsigned cp) {
        if (cp < 0x80u) {
            out += (char)cp;
        } else if (cp < 0x800u) {
            out += (char)(0xc0u | (cp >> 6));
            out += (char)(0x80u | (cp & 0x3fu));
        } else if (cp < 0x10000u) {
            out += (char)(0xe0u | (cp >> 12));
            out += (char)(0x80u | ((cp >> 6) & 0x3fu));
            out += (char)(0x80u | (cp & 0x3fu));
        } else {
            out += (char)(0xf0u | (cp >> 18));
            out += (char)(0x80u | ((cp >> 12) & 0x3fu));
            out += (char)(0x80u | ((cp >> 6) & 0x3fu));
            out += (char)(0x80u | (cp & 0x3fu));
        }
    }
    // one UTF-8 sequence of two to four bytes at p, copied: shortest form, no surrogate, at most U+10FFFF
    void utf8(std::string &out) {
        const unsigned char c = s[p];
        const size_t len = c >= 0xf0u ? 4 : c >= 0xe0u ? 3 : 2;
        if (c < 0xc2u || c > 0xf4u || n - p < len) fail("invalid UTF-8");
        unsigned cp = c & (0xffu >> (len + 1));
        for (size_t k = 1; k < len; ++k) {
            if ((s[p + k] & 0xc0u) != 0x80u) fail("invalid UTF-8");
            cp = (cp << 6) | (s[p + k] & 0x3fu);
        }
        if ((len == 3 && cp < 0x800u) || (len == 4 && cp < 0x10000u) || (cp >= 0xd800u && cp <= 0xdfffu) || cp > 0x10ffffu)
            fail("invalid UTF-8");
        out.append(reinterpret_cast<const char *>(s + p), len);
        p += len;
    }
    // the string whose opening quote is at p
    std::string str() {
        std::string out;
        ++p;
        for (;;) {
            if (p >= n) fail("an unterminated string");
            const unsigned char c = s[p];
            if (c == '"') {
                ++p;
                return out;
            }
            if (c < 0x20u) fail("a control character in a string");
            if (c >= 0x80u) {
                utf8(out);
                continue;
            }
            ++p;
            if (c != '\\') {
                out += (char)c;
                continue;
            }
            if (p >= n) fail("an unterminated string");
            const unsigned char e = s[p++];
            switch (e) {
                case '"': out += '"'; break;
                case '\\': out += '\\'; break;
                case '/': out += '/'; break;
                case 'b': out += '\b'; break;
                case 'f': out += '\f'; break;
                case 'n': out += '\n'; break;
                case 'r': out += '\r'; break;
                case 't': out += '\t'; break;
                case 'u': {
                    unsigned cp = hex4();
                    if (cp >= 0xdc00u && cp <= 0xdfffu) fail("a lone surrogate");
                    if (cp >= 0xd800u && cp <= 0xdbffu) {
                        if (n - p < 2 || s[p] != '\\' || s[p + 1] != 'u') fail("a lone surrogate");
                        p += 2;
                        const unsigned lo = hex4();
                        if (lo < 0xdc00u || lo > 0xdfffu) fail("a lone surrogate");
                        cp = 0x10000u + ((cp - 0xd800u) << 10) + (lo - 0xdc00u);
                    }
                    put_utf8(out, cp);
                    break;
                }
                default: fail("an unknown escape");
            }
        }
    }
};

// an optional '-' and decimal digits at t[p ..), inside i32
int32_t runlist_int(const std::string &t, size_t &p) {
    const bool neg = p < t.size() && t[p] == '-';
    if (neg) ++p;
    const size_t b = p;
    int64_t v = 0;
    while (p < t.size() && t[p] >= '0' && t[p] <= '9') {
        v = v * 10 + (t[p] - '0');
        if (v > 2147483648ll) throw Error(GAMS_EINVAL, "read_runlist_json: a number outside i32 in '" + t + "'");
        ++p;
    }
    if (p == b) throw Error(GAMS_EINVAL, "read_runlist_json: a token without a number in '" + t + "'");
    if (neg) v = -v;
    if (v > 2147483647ll) throw Error(GAMS_EINVAL, "read_runlist_json: a number outside i32 in '" + t + "'");
    return (int32_t)v;
}

}  // namespace

Runlist parse_runlist(const std::string &text) {
    Runlist raw;
    for (const char c : text)
        if (!((c >= '0' && c <= '9') || c == '-' || c == ','))
            throw Error(GAMS_EINVAL, "read_runlist_json: a runlist character that is no digit, '-' or ',' in '" + text + "'");
    if (text.empty() || text == "-") return raw;
    size_t b = 0;
    while (b <= text.size()) {
        const size_t e = std::min(text.find(',', b), text.size());
        if (e > b) {
            const std::string tok = text.substr(b, e - b);
            size_t p = 0;
            const int32_t lo = runlist_int(tok, p);
            int32_t hi = lo;
            if (p < tok.size()) {
                ++p;                                  // the '-' between the numbers (the only byte it can be)
                hi = runlist_int(tok, p);
            }
            if (p != tok.size()) throw Error(GAMS_EINVAL, "read_runlist_json: a token that is not a or a-b: '" + tok + "'");
            if (lo > hi) throw Error(GAMS_EINVAL, "read_runlist_json: a span with a > b: '" + tok + "'");
            raw.lo.push_back(lo);
            raw.hi.push_back(hi);
        }
        b = e + 1;
    }
    // IntSpan::add_runlist: the union, overlapping and adjacent spans joined
    std::vector<size_t> order(raw.lo.size());
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return raw.lo[x] < raw.lo[y]; });
    Runlist out;
    for (const size_t i : order) {
        if (!out.lo.empty() && (int64_t)raw.lo[i] <= (int64_t)out.hi.back() + 1)
            out.hi.back() = std::max(out.hi.back(), raw.hi[i]);
        else {
            out.lo.push_back(raw.lo[i]);
            out.hi.push_back(raw.hi[i]);
        }
    }
    return out;
}

RunlistJson read_runlist_json(const char *bytes, size_t n) {
    JsonIn in{reinterpret_cast<const unsigned char *>(bytes ? bytes : ""), n};
    RunlistJson out;
    std::map<std::string, size_t> place;
    in.ws();
    if (in.p >= n || in.s[in.p] != '{') in.fail("not an object");
    ++in.p;
    in.ws();
    if (in.p < n && in.s[in.p] == '}') {
        ++in.p;
    } else {
        for (;;) {
            in.ws();
            if (in.p >= n || in.s[in.p] != '"') in.fail("a key is expected");
            const std::string key = in.str();
            in.ws();
            if (in.p >= n || in.s[in.p] != ':') in.fail("a ':' is expected");
            ++in.p;
            in.ws();
            if (in.p >= n || in.s[in.p] != '"') in.fail("a value that is not a string");
            const Runlist set = parse_runlist(in.str());
            const auto at = place.find(key);
            if (at == place.end()) {
                place[key] = out.chr.size();
                out.chr.push_back(key);
                out.sets.push_back(set);
            } else {
                out.sets[at->second] = set;           // the last value wins, the key keeps its place
            }
            in.ws();
            if (in.p < n && in.s[in.p] == ',') {
                ++in.p;
                continue;
            }
            if (in.p < n && in.s[in.p] == '}') {
                ++in.p;
                break;
            }
            in.fail("a ',' or a '}' is expected");
        }
    }
    in.ws();
    if (in.p != n) in.fail("text behind the object");
    return out;
}

}  // namespace gams
