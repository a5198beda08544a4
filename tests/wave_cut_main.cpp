// Stand-alone driver of wave_select_cut() (gams_amd/csrc/wave_select.hpp) for tests/test_wave_cut_cpu.py (host compiler,
// no HIP).  Reads the cases of wave_select_main.cpp from stdin with the cut request in front, one per line:
//     cut_req size step lag flags serial repair depth total_windows tw_req nth_req taper_req cus set_bytes
// and prints per case, tab-separated:
//     kernel narrow body_nth body_w body_lds_bytes | cut cut_nth cut_w cut_lds_bytes | onewave_bm_bytes onewave_k_bytes pad
#include <iostream>

#include "../gams_amd/csrc/wave_select.hpp"

int main() {
    char name[128];
    long long cut_req, size, step, lag, flags, serial, repair, depth, total, tw_req, nth_req, taper_req, cus, bytes;
    while (std::cin >> cut_req >> size >> step >> lag >> flags >> serial >> repair >> depth >> total >> tw_req >> nth_req >>
           taper_req >> cus >> bytes) {
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
        const WaveBody b = wave_select_body(in, s);
        const WaveCut c = wave_select_cut(b, (int)cut_req);
        wave_selection_name(s, name, sizeof name);
        std::printf("%s\t%d\t%u\t%u\t%zu\t%d\t%u\t%u\t%zu\t%zu\t%zu\t%u\n", name, (int)b.narrow, b.nth, b.w, b.lds_bytes, c.cut, c.nth,
                    c.w, c.lds_bytes, wave_onewave_bm_bytes(), wave_onewave_k_bytes(), kWaveOneWavePad);
    }
    return 0;
}
