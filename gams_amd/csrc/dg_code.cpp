// dg_code.cpp -- the host side of the nearest-neighbour ΔG (src/libs/delta_g.rs): the table of a (temp, salt) pair and the
// host twin of the device entries, over the code map the kernel shares (dg_code.hpp).  Plain C++, built with
// -ffp-contract=off: every step below is one f32 operation, in the reference's order.
#include "dg_code.hpp"

#include <cmath>
#include <limits>

#include "../../include/gams_gpu.h"

namespace {
// SantaLucia 1998, unified parameters: ΔH (kcal/mol) and ΔS (cal/K.mol) of the dimer XY at 4 * c(X) + c(Y)
// (delta_g.rs:120-171)
const float kDh[16] = {-7.6f, -8.4f, -7.8f, -7.2f, -8.5f, -8.0f, -10.6f, -7.8f,
                       -8.2f, -9.8f, -8.0f, -8.4f, -7.2f, -8.2f, -8.5f, -7.6f};
const float kDs[16] = {-21.3f, -22.4f, -21.0f, -20.4f, -22.7f, -19.9f, -27.2f, -21.0f,
                       -22.2f, -24.4f, -19.9f, -22.4f, -21.3f, -22.2f, -22.7f, -21.3f};
}  // namespace

// delta_g.rs:179-206: the terminal and symmetry terms are constants, a dimer's is dH - T * dS with the salt in dS
extern "C" int gams_dg_table(float temp, float salt, gams_dg_table_t *t) {
    if (!t || !std::isfinite(temp) || !std::isfinite(salt) || !(salt > 0.0f)) return GAMS_EINVAL;
    const float adj = 0.368f * logf(salt);
    for (int i = 0; i < 16; ++i) {
        const float ds = kDs[i] + adj;
        t->nn[i] = kDh[i] - ((273.15f + temp) * (ds / 1000.0f));
    }
    t->init[0] = t->init[3] = 0.05f;
    t->init[1] = t->init[2] = 1.96f;
    t->sym = 0.43f;
    return GAMS_OK;
}

// delta_g.rs:78-115
extern "C" int gams_dg_polymer_host(const gams_dg_table_t *t, const uint8_t *seq, uint64_t n, float *dg) {
    if (!t || !dg || (n && !seq)) return GAMS_EINVAL;
    *dg = std::numeric_limits<float>::quiet_NaN();
    if (n < 3) return GAMS_OK;
    for (uint64_t i = 0; i < n; ++i)
        if (dg_code1(seq[i]) > 3u) return GAMS_OK;
    float v = 0.0f;
    uint32_t prev = dg_code1(seq[0]);
    const uint32_t first = prev;
    for (uint64_t i = 1; i < n; ++i) {
        const uint32_t cur = dg_code1(seq[i]);
        v += t->nn[4u * prev + cur];
        prev = cur;
    }
    v += t->init[first];
    v += t->init[prev];
    bool sym = (n & 1u) == 0;
    for (uint64_t i = 0; sym && i < n / 2; ++i) sym = dg_code1(seq[i]) + dg_code1(seq[n - 1 - i]) == 3u;
    if (sym) v += t->sym;
    *dg = v;
    return GAMS_OK;
}
