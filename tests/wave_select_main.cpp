// Stand-alone driver of gams_amd/csrc/wave_select.hpp for tests/test_wave_select_cpu.py (host compiler, no HIP).
//   wave_select_main list      the name of every entry of the instance list, NT = false (the `true` half differs in that word)
//   wave_select_main           reads cases from stdin, one per line:
//                                size step lag flags serial repair depth total_windows tw_req nth_req taper_req cus set_bytes
//                              prints per case, tab-separated:
//                                kernel nth tw max_win max_chunks lds_bytes taper direct
//   wave_select_main taper     reads batches from stdin (tests/test_wave_taper_cpu.py), one per line:
//                                cus pct4 pct8 lag n_ctg  then the n_ctg window counts of the batch's ctgs
//                              prints per batch one line: the two tail sizes x4 y8, then per ctg its tile width and tiles
#include <cstring>
#include <iostream>
#include <vector>

#include "../gams_amd/csrc/wave_select.hpp"

int main(int argc, char **argv) {
    char name[128];
    if (argc > 1 && std::strcmp(argv[1], "list") == 0) {
        WaveSelection s;
        s.family = kWaveFamFast;
        for (s.entry = 0; s.entry < kWaveFastCount; ++s.entry) {
            wave_selection_name(s, name, sizeof name);
            std::printf("%s\n", name);
        }
        return 0;
    }
    if (argc > 1 && std::strcmp(argv[1], "taper") == 0) {
        long long cus, pct4, pct8, lag, n;
        while (std::cin >> cus >> pct4 >> pct8 >> lag >> n) {
            std::vector<unsigned long long> win((size_t)n);
            unsigned long long total = 0;
            for (auto &w : win) {
                std::cin >> w;
                total += w;
            }
            const WaveTaper t = wave_taper_tails(total, wave_slots((int)cus), (uint32_t)lag, (int)pct4, (int)pct8);
            std::printf("%llu %llu", (unsigned long long)t.x4, (unsigned long long)t.y8);
            unsigned long long base = 0;
            for (unsigned long long w : win) {
                const uint32_t kind = wave_taper_width(t, total - base);
                const uint32_t tw = wave_taper_tile_windows(t, kind);
                std::printf(" %u %llu", kind, (w + tw - 1) / tw);
                base += w;
            }
            std::printf("\n");
        }
        return 0;
    }
    long long size, step, lag, flags, serial, repair, depth, total, tw_req, nth_req, taper_req, cus, bytes;
    while (std::cin >> size >> step >> lag >> flags >> serial >> repair >> depth >> total >> tw_req >> nth_req >> taper_req >> cus >> bytes) {
        WaveSelectIn in{};
        in.prm = gams_wave_params_t{(int32_t)size, (int32_t)step, (uint32_t)lag, 3.0f, serial ? 0.5f : 1.0f};
        in.flags = (uint32_t)flags;
        in.serial = serial != 0;
        in.repair = repair != 0;
        in.depth = (uint32_t)depth;
        in.total_windows = (uint64_t)total;
        in.tw_req = (uint32_t)tw_req;
        in.nth_req = (uint32_t)nth_req;
        in.taper_req = (int)taper_req;
        in.cus = (int)cus;
        in.set_bytes = (uint64_t)bytes;
        WaveSelection s;
        if (!wave_select(in, s)) {
            std::printf("NONE\n");
            continue;
        }
        wave_selection_name(s, name, sizeof name);
        std::printf("%s\t%u\t%u\t%u\t%u\t%zu\t%d\t%d\n", name, s.nth, s.tw, s.max_win, s.max_chunks, s.lds_bytes, (int)s.taper,
                    (int)s.direct);
    }
    return 0;
}
