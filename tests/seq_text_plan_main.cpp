// Stand-alone driver of gams_amd/csrc/seq_text_plan.hpp for tests/test_locate_seq_text_cpu.py (host compiler, no HIP; built
// with -fsanitize=address,undefined).  `--chunk` prints kSeqTextChunk.  Otherwise every line of stdin is one set of rows,
// tokens separated by blanks: "x" is a line without a row, "R:B" a row with R bytes of rg and B bases.  The rows' bytes are
// made up here; every chunk of the text is then copied run by run, with memcpy, into a zero-filled buffer that has guard
// bytes on both sides, and per set one line is printed:
//     ok <total> <chunks> <runs> <begin_mask> <end_mask>      or      FAIL <what>
// begin_mask / end_mask: bit p is set if a piece p began on the first byte of a chunk / ended on the last byte of a chunk
// that is full (a seam, not the end of the text).
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../gams_amd/csrc/seq_text_plan.hpp"

namespace {

constexpr size_t kGuard = 64;
constexpr unsigned char kGuardByte = 0xa5;

struct Rows {
    std::vector<uint64_t> row_off, rg_len, n_bases, rg_at, bases_at;   // row_off: rows + 1
    std::string in, seq;                                               // what the rg and the bases pieces are copied from
};

std::string run_set(const Rows &R) {
    const uint64_t n = R.rg_len.size(), total = R.row_off[n];
    std::string want;
    for (uint64_t r = 0; r < n; ++r) {
        if (R.row_off[r + 1] == R.row_off[r]) continue;
        want += '>';
        want += R.in.substr(R.rg_at[r], R.rg_len[r]);
        want += '\n';
        want += R.seq.substr(R.bases_at[r], R.n_bases[r]);
        want += '\n';
    }
    if (want.size() != total) return "FAIL the rows do not add up to the total";
    std::vector<unsigned char> buf(kGuard + total + kGuard, 0);
    memset(buf.data(), kGuardByte, kGuard);
    memset(buf.data() + kGuard + total, kGuardByte, kGuard);
    unsigned char *const text = buf.data() + kGuard;
    uint64_t next = 0, runs = 0;
    unsigned begin_mask = 0, end_mask = 0;
    const uint64_t chunks = seq_plan_chunks(total);
    for (uint64_t k = 0; k < chunks; ++k) {
        const uint64_t c0 = seq_plan_chunk_begin(k), c1 = seq_plan_chunk_end(k, total);
        if (c0 % 16 != 0 || c0 >= c1 || c1 - c0 > kSeqTextChunk) return "FAIL a chunk is not a chunk";
        uint64_t r = seq_plan_row_at(R.row_off.data(), 0, n, c0);
        for (uint64_t pos = c0; pos < c1;) {
            if (r >= n || R.row_off[r] > pos || pos >= R.row_off[r + 1]) return "FAIL the row found does not hold the byte";
            const SeqRun u = seq_plan_run(R.row_off[r], R.rg_len[r], R.n_bases[r], pos, c1);
            if (u.len == 0) return "FAIL an empty run";
            if (u.dst_off != next) return "FAIL the runs do not tile the text in order";
            if (u.dst_off < c0 || u.dst_off + u.len > c1) return "FAIL a run crosses its chunk";
            const char one = u.piece == SEQ_GT ? '>' : '\n';
            const char *src = &one;
            uint64_t piece_len = 1;
            if (u.piece == SEQ_RG) src = R.in.data() + R.rg_at[r], piece_len = R.rg_len[r];
            if (u.piece == SEQ_BASES) src = R.seq.data() + R.bases_at[r], piece_len = R.n_bases[r];
            if (u.piece >= SEQ_PIECES || u.src_off + u.len > piece_len) return "FAIL a run leaves its piece";
            memcpy(text + u.dst_off, src + u.src_off, u.len);
            if (u.src_off == 0 && u.dst_off == c0) begin_mask |= 1u << u.piece;
            if (u.src_off + u.len == piece_len && u.dst_off + u.len == c1 && c1 - c0 == kSeqTextChunk) end_mask |= 1u << u.piece;
            next = pos = u.dst_off + u.len;
            ++runs;
            if (pos == R.row_off[r + 1] && pos < total) {
                const uint64_t nr = seq_plan_next_row(R.row_off.data(), r, n, pos);
                if (nr != seq_plan_row_at(R.row_off.data(), r + 1, n, pos)) return "FAIL the next row is not the row the search finds";
                r = nr;
            }
        }
    }
    if (next != total) return "FAIL the runs end before the text does";
    for (size_t g = 0; g < kGuard; ++g)
        if (buf[g] != kGuardByte || buf[kGuard + total + g] != kGuardByte) return "FAIL a guard byte was written";
    if (memcmp(text, want.data(), total) != 0) return "FAIL the text differs from the rows one after the other";
    std::ostringstream os;
    os << "ok " << total << ' ' << chunks << ' ' << runs << ' ' << begin_mask << ' ' << end_mask;
    return os.str();
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "--chunk") {
        std::printf("%u\n", kSeqTextChunk);
        return 0;
    }
    std::string line;
    uint32_t lcg = 12345u;
    auto next_byte = [&] {
        lcg = lcg * 1664525u + 1013904223u;
        return (char)(lcg >> 24);
    };
    while (std::getline(std::cin, line)) {
        Rows R;
        R.row_off.push_back(0);
        std::istringstream is(line);
        std::string tok;
        while (is >> tok) {
            uint64_t rg = 0, nb = 0, len = 0;
            if (tok != "x") {
                const size_t colon = tok.find(':');
                if (colon == std::string::npos) {
                    std::printf("FAIL a token is neither x nor R:B\n");
                    return 1;
                }
                rg = std::stoull(tok.substr(0, colon));
                nb = std::stoull(tok.substr(colon + 1));
                len = seq_plan_row_len(rg, nb);
            }
            R.rg_len.push_back(rg);
            R.n_bases.push_back(nb);
            R.rg_at.push_back(R.in.size());
            R.bases_at.push_back(R.seq.size());
            if (len) {
                for (uint64_t q = 0; q < rg; ++q) R.in += next_byte();
                for (uint64_t q = 0; q < nb; ++q) R.seq += next_byte();
            }
            R.row_off.push_back(R.row_off.back() + len);
        }
        std::printf("%s\n", run_set(R).c_str());
    }
    return 0;
}
