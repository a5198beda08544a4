// gams_sw_summary.cpp -- the host half of the sw summary: the summariser of rows that came back as arrays,
// the table's header and its text.  Plain C++17, no device call: the stand-alone driver tests/sw_anno_summary_main.cpp
// links this unit alone.
#include <cmath>
#include <cstdio>

#include "../csrc/text_fmt.hpp"
#include "gams_host.hpp"

namespace gams {

uint32_t prop4_units(float p) {
    if (!(p >= 0.0f && p <= 1.0f)) throw Error(GAMS_EINVAL, "prop4_units: not a value in [0, 1]");
    return gams_prop4_units(p);
}

void sw_summarise_rows(const gams_sw_row_t *rows, const int32_t *counts, uint64_t n, int32_t max, uint32_t actions,
                       uint64_t *table, uint32_t n_props, const uint32_t *const *props, uint64_t *prop_table) {
    const bool do_gc = (actions & GAMS_SW_GC) != 0, do_count = (actions & GAMS_SW_COUNT) != 0;
    if (do_count && n && !counts) throw Error(GAMS_EINVAL, "sw_summarise_rows: GAMS_SW_COUNT without the counts");
    if (n_props && (!props || !prop_table)) throw Error(GAMS_EINVAL, "sw_summarise_rows: Prop columns without their units or table");
    for (uint32_t a = 0; a < n_props; ++a)
        if (n && !props[a]) throw Error(GAMS_EINVAL, "sw_summarise_rows: a null column of Prop units");
    for (uint64_t r = 0; r < n; ++r) {
        const gams_sw_row_t &w = rows[r];
        if (w.distance < 0 || w.distance > max) throw Error(GAMS_EINVAL, "sw_summarise_rows: a distance outside [0, max]");
        uint64_t *g = table + (size_t)w.distance * GAMS_SW_SUMMARY_WORDS;
        g[0] += 1;
        if (do_gc) {
            const float v[4] = {w.gc_content, w.gc_mean, w.gc_stddev, w.gc_cv};
            for (int k = 0; k < 4; ++k) {
                if (v[k] != v[k])
                    g[5 + k] += 1;
                else if (!(v[k] >= 0.0f) || std::isinf(v[k]))
                    throw Error(GAMS_EUNSUPPORTED, "sw_summarise_rows: a negative or infinite statistic has no place in the table");
                else   // the integer nearest to v * 10^4 -- below 1000 the m the text prints (sw_put_f4), beyond it its continuation
                    g[1 + k] += (uint64_t)((double)v[k] * 10000.0 + 0.5);
            }
        }
        if (do_count) g[9] += (uint64_t)(int64_t)counts[r];
        for (uint32_t a = 0; a < n_props; ++a) {
            if (props[a][r] > 10000u) throw Error(GAMS_EINVAL, "sw_summarise_rows: Prop units beyond 10000");
            prop_table[(size_t)w.distance * n_props + a] += props[a][r];
        }
    }
}

std::string sw_summary_header(uint32_t actions, bool tagged, const std::vector<std::string> &prefixes) {
    std::string o = tagged ? "tag\tdistance" : "distance";
    if (actions & GAMS_SW_GC) o += "\tAVG_gc_content\tAVG_gc_mean\tAVG_gc_stddev\tAVG_gc_cv";
    for (const std::string &p : prefixes) o += "\tAVG_" + p + "Prop";
    if (actions & GAMS_SW_COUNT) o += "\tAVG_rg_count";
    return o + "\tCOUNT\n";
}

namespace {
// num / den to the nearest integer, ties to even, printed as q / 10^4 with the trailing zeros dropped (as sw_put_f4 prints)
std::string sw_avg4(unsigned __int128 num, uint64_t den) {
    unsigned __int128 q = num / den;
    const unsigned __int128 r2 = (num % den) * 2;
    if (r2 > den || (r2 == den && (q & 1))) ++q;
    std::string ip, o;
    unsigned __int128 i = q / 10000;
    do {
        ip.insert(ip.begin(), (char)('0' + (int)(i % 10)));
        i /= 10;
    } while (i);
    uint32_t fr = (uint32_t)(q % 10000), nd = 4;
    while (nd && fr % 10 == 0) {
        fr /= 10;
        --nd;
    }
    o = ip;
    if (nd) {
        char buf[8];
        std::snprintf(buf, sizeof buf, ".%0*u", (int)nd, fr);
        o += buf;
    }
    return o;
}
}  // namespace

std::string SwSummaryTable::text() const {
    const bool tagged = !tags.empty();
    std::string o = sw_summary_header(actions, tagged, prefixes);
    const size_t n_tags = tagged ? tags.size() : 1, n_anno = prefixes.size();
    for (size_t t = 0; t < n_tags; ++t)
        for (int32_t d = 0; d <= max; ++d) {
            const size_t gi = t * ((size_t)max + 1) + (size_t)d;
            const uint64_t *g = words.data() + gi * GAMS_SW_SUMMARY_WORDS;
            if (g[0] == 0) continue;
            if (tagged) o += tags[t] + "\t";
            o += std::to_string(d);
            if (actions & GAMS_SW_GC)
                for (int k = 0; k < 4; ++k) o += "\t" + (g[5 + k] ? std::string("nan") : sw_avg4(g[1 + k], g[0]));
            for (size_t a = 0; a < n_anno; ++a) o += "\t" + sw_avg4(prop[gi * n_anno + a], g[0]);
            if (actions & GAMS_SW_COUNT) o += "\t" + sw_avg4((unsigned __int128)g[9] * 10000u, g[0]);
            o += "\t" + std::to_string(g[0]) + "\n";
        }
    return o;
}

}  // namespace gams
