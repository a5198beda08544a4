// sw_anno_summary_main.cpp -- stand-alone driver of the host half of the sw summary (gams_amd/host/gams_sw_summary.cpp)
// and of the prop formatter both sides share (gams_amd/csrc/text_fmt.hpp), built by tests/test_sw_anno_summary_cpu.py
// with the address and undefined-behaviour sanitizers: no HIP, no device.
//
//   sw_anno_summary_main <file>
// <file>: a first line "max actions n_props prefix..." and one line per row, "distance gc_content gc_mean gc_stddev gc_cv
// count q..." (a statistic as a decimal or "nan"; n_props Prop units).  The rows go through gams::sw_summarise_rows from
// heap blocks of exactly their size and the table is printed with SwSummaryTable::text.  In front of it the driver prints
// "units <n>": for every (card, len) with 1 <= len <= 600 and 0 <= card <= len, gams_prop4_units of the f32 quotient
// agrees with the digits of gams_fmt_prop4 and with "%.4f" of the widened value (n pairs; a disagreement exits 1).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../gams_amd/csrc/text_fmt.hpp"
#include "../gams_amd/host/gams_host.hpp"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    unsigned pairs = 0;
    for (int len = 1; len <= 600; ++len)
        for (int card = 0; card <= len; ++card, ++pairs) {
            const float p = (float)card / (float)len;
            char a[8] = {0}, b[16];
            if (!gams_fmt_prop4(p, a)) return 1;
            std::snprintf(b, sizeof b, "%.4f", (double)p);
            const uint32_t q = gams_prop4_units(p);
            char c[16];
            std::snprintf(c, sizeof c, "%u.%04u", q / 10000u, q % 10000u);
            if (std::strcmp(a, b) != 0 || std::strcmp(a, c) != 0 || gams::prop4_units(p) != q) {
                std::fprintf(stderr, "prop4 %d/%d: %s %s %s\n", card, len, a, b, c);
                return 1;
            }
        }
    std::printf("units %u\n", pairs);

    std::ifstream fh(argv[1]);
    std::string line;
    if (!std::getline(fh, line)) return 2;
    std::istringstream head(line);
    int32_t max = 0;
    uint32_t actions = 0, n_props = 0;
    head >> max >> actions >> n_props;
    gams::SwSummaryTable T;
    T.max = max;
    T.actions = actions;
    for (uint32_t a = 0; a < n_props; ++a) {
        std::string p;
        head >> p;
        T.prefixes.push_back(p);
    }
    std::vector<gams_sw_row_t> rows;
    std::vector<int32_t> counts;
    std::vector<std::vector<uint32_t>> props(n_props);
    while (std::getline(fh, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        gams_sw_row_t r{};
        std::string f[4];
        int32_t cnt = 0;
        in >> r.distance >> f[0] >> f[1] >> f[2] >> f[3] >> cnt;
        float *v[4] = {&r.gc_content, &r.gc_mean, &r.gc_stddev, &r.gc_cv};
        for (int k = 0; k < 4; ++k) *v[k] = std::strtof(f[k].c_str(), nullptr);
        for (uint32_t a = 0; a < n_props; ++a) {
            uint32_t q = 0;
            in >> q;
            props[a].push_back(q);
        }
        rows.push_back(r);
        counts.push_back(cnt);
    }
    // exact-size heap blocks: a read past a column's end is the sanitizer's to report
    const size_t n = rows.size();
    std::unique_ptr<gams_sw_row_t[]> hr(new gams_sw_row_t[n]);
    std::unique_ptr<int32_t[]> hc(new int32_t[n]);
    std::vector<std::unique_ptr<uint32_t[]>> hp;
    std::vector<const uint32_t *> pp;
    for (size_t i = 0; i < n; ++i) hr[i] = rows[i], hc[i] = counts[i];
    for (uint32_t a = 0; a < n_props; ++a) {
        hp.emplace_back(new uint32_t[n]);
        for (size_t i = 0; i < n; ++i) hp.back()[i] = props[a][i];
        pp.push_back(hp.back().get());
    }
    T.words.assign(((size_t)max + 1) * GAMS_SW_SUMMARY_WORDS, 0);
    T.prop.assign(((size_t)max + 1) * n_props, 0);
    try {
        gams::sw_summarise_rows(hr.get(), hc.get(), n, max, actions, T.words.data(), n_props, pp.data(), T.prop.data());
    } catch (const gams::Error &e) {
        std::printf("error %d\n", e.code);
        return 0;
    }
    std::fputs(T.text().c_str(), stdout);
    return 0;
}
