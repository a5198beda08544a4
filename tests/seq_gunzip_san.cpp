// seq_gunzip_san.cpp -- the shared decoder core of the indexed `seq:` members (gams_amd/csrc/seq_gunzip_code.hpp) over a
// corpus of members and a sweep of single-bit flips, as a stand-alone program for a sanitizer build
// (tests/test_seq_gz_index_cpu.py compiles it with -fsanitize=address,undefined and compares what it prints with the
// library's answers).  Every member is decoded out of a heap block of exactly its size, into one of exactly ISIZE
// bytes, so a load or a store one byte outside either is reported.
//   seq_gunzip_san CORPUS [SWEPT FLIPS]
// CORPUS: members as (u64 length, bytes) records.  FLIPS: u64 bit positions, each flipped on its own in a copy of
// member number SWEPT.  One line per decode: status, bases, their FNV-1a hash.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gams_amd/csrc/seq_gunzip_code.hpp"

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    uint8_t buf[1 << 16];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) != 0;) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

static void decode(const uint8_t *member, uint64_t n) {
    uint8_t *exact = static_cast<uint8_t *>(std::malloc(n ? n : 1));
    std::memcpy(exact, member, n);
    uint32_t isize = 0;
    if (n >= 4) std::memcpy(&isize, member + n - 4, 4);
    const uint64_t cap = isize < (1u << 26) ? isize : (1u << 26);
    uint8_t *out = static_cast<uint8_t *>(std::malloc(cap ? cap : 1));
    uint64_t n_out = 0;
    int status = -1;
    const bool fits = gams_gunzip::gunzip_member(exact, n, out, cap, &n_out, &status);
    uint64_t h = 1469598103934665603ull;
    if (fits && status == gams_gunzip::kDone)
        for (uint64_t i = 0; i < n_out; ++i) h = (h ^ out[i]) * 1099511628211ull;
    std::printf("%d %" PRIu64 " %016" PRIx64 "\n", fits ? status : -1, n_out, fits && status == gams_gunzip::kDone ? h : 0);
    std::free(out);
    std::free(exact);
}

int main(int argc, char **argv) {
    if (argc != 2 && argc != 4) {
        std::fprintf(stderr, "usage: %s CORPUS [SWEPT FLIPS]\n", argv[0]);
        return 2;
    }
    const std::vector<uint8_t> corpus = slurp(argv[1]);
    std::vector<std::pair<size_t, uint64_t>> members;
    for (size_t at = 0; at + 8 <= corpus.size();) {
        uint64_t n;
        std::memcpy(&n, corpus.data() + at, 8);
        if (n > corpus.size() - at - 8) return 2;
        members.push_back({at + 8, n});
        at += 8 + n;
    }
    for (const auto &m : members) decode(corpus.data() + m.first, m.second);
    if (argc == 4) {
        const size_t which = (size_t)std::strtoull(argv[2], nullptr, 10);
        if (which >= members.size()) return 2;
        const std::vector<uint8_t> flips = slurp(argv[3]);
        std::vector<uint8_t> copy(corpus.begin() + (long)members[which].first,
                                  corpus.begin() + (long)(members[which].first + members[which].second));
        for (size_t at = 0; at + 8 <= flips.size(); at += 8) {
            uint64_t bit;
            std::memcpy(&bit, flips.data() + at, 8);
            if ((bit >> 3) >= copy.size()) return 2;
            copy[bit >> 3] ^= (uint8_t)(1u << (bit & 7u));
            decode(copy.data(), copy.size());
            copy[bit >> 3] ^= (uint8_t)(1u << (bit & 7u));
        }
    }
    return 0;
}
