// runlist_main.cpp -- stand-alone driver of the host reader of runlist JSON files (gams_amd/host/gams_runlist.cpp),
// built by tests/test_runlist_text_cpu.py with the address and undefined-behaviour sanitizers: no HIP, no device.
//
//   runlist_main <file>
// <file> holds documents back to back, each as a 4-byte little-endian length and its bytes.  For document i the driver
// prints "D <i> E" where the reader answers GAMS_EINVAL, else "D <i> A <set>" with <set> = the groups joined by ';',
// each the key in hex, '=', and its spans "lo:hi" joined by ','; then "T <i> <verdicts>", one letter (A or E) for the
// document cut to its first k bytes, k = 0 .. length - 1.  Every cut is read from a heap block of exactly k bytes, so
// that a read past the end is the sanitizer's to report.  Exit status 0 unless the reader throws anything else.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../gams_amd/host/gams_host.hpp"

namespace {

std::string show(const gams::RunlistJson &js) {
    static const char *hex = "0123456789abcdef";
    std::string out;
    for (size_t g = 0; g < js.chr.size(); ++g) {
        if (g) out += ';';
        for (const unsigned char c : js.chr[g]) {
            out += hex[c >> 4];
            out += hex[c & 15];
        }
        out += '=';
        for (size_t i = 0; i < js.sets[g].lo.size(); ++i) {
            if (i) out += ',';
            out += std::to_string(js.sets[g].lo[i]) + ":" + std::to_string(js.sets[g].hi[i]);
        }
    }
    return out;
}

// 'A' + the set, or 'E'; anything but GAMS_EINVAL leaves through main
std::string read(const char *bytes, size_t n, bool with_set) {
    try {
        const gams::RunlistJson js = gams::read_runlist_json(bytes, n);
        return with_set ? "A " + show(js) : "A";
    } catch (const gams::Error &e) {
        if (e.code != GAMS_EINVAL) throw;
        return "E";
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream fh(argv[1], std::ios::binary);
    const std::string all((std::istreambuf_iterator<char>(fh)), std::istreambuf_iterator<char>());
    size_t at = 0;
    for (unsigned i = 0; at + 4 <= all.size(); ++i) {
        uint32_t len = 0;
        std::memcpy(&len, all.data() + at, 4);
        at += 4;
        if (len > all.size() - at) return 3;
        const std::vector<char> whole(all.begin() + at, all.begin() + at + len);
        std::printf("D %u %s\n", i, read(whole.data(), whole.size(), true).c_str());
        std::string cuts;
        for (size_t k = 0; k < len; ++k) {
            const std::vector<char> cut(whole.begin(), whole.begin() + k);
            cuts += read(cut.data(), cut.size(), false);
        }
        std::printf("T %u %s\n", i, cuts.c_str());
        at += len;
    }
    return 0;
}
