// gen_split.hpp -- what the device path of `gams gen` (gen.hip) and the host layer (host/gams_host.cpp) must agree on.
// Plain C++17 (no HIP).
#pragma once

#include <cstdint>

// ASCII white space as Rust's char::is_whitespace sees it below 0x80: what ends a FASTA id and what the reference's
// trim_end() drops from a line
inline bool gams_fasta_space(uint8_t c) { return c == ' ' || (c >= 0x09 && c <= 0x0d); }

// gen.rs:108-126: the valid span [pos, max] (1-based, inclusive) in pieces of `piece` bases while more than `piece`
// remain, the last piece absorbing the remainder; emit(start, end) per piece, in order
template <typename Emit>
void gams_piece_split(int64_t pos, int64_t max, int32_t piece, Emit emit) {
    while (max - pos + 1 > 2 * (int64_t)piece) {
        emit(pos, pos + piece - 1);
        pos += piece;
    }
    emit(pos, max);
}
