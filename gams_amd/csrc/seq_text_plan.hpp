// seq_text_plan.hpp -- where the bytes of the `locate --seq` text come from (gams_gpu_locate_seq_text, text.hip).
//
// Plain C++17, no HIP: the copy kernel and tests/seq_text_plan_main.cpp (host compiler, sanitizers) include the same
// arithmetic.  Everything is constexpr, so the device compiler takes it as it stands.
//
// The text is the rows of the located lines, in line order: row r begins at byte row_off[r] (row_off has one entry per
// line and the total behind them; a line without a row has a row of zero bytes) and is five pieces,
//     '>' | rg (rg_len bytes of the input) | '\n' | bases (n_bases bytes of the seqset) | '\n'
// The text is cut into chunks of kSeqTextChunk bytes, one workgroup each; a chunk begins on a multiple of kSeqTextChunk,
// hence on a 16-B boundary, so its 16-B units are the text's.  A run is a stretch of one piece of one row inside one
// stretch [pos, end) of the text: whoever copies [pos, end) -- a chunk on the host, a 16-B unit on the device -- asks for
// the row at pos, then for run after run until end, and for the next row wherever a run ends its row.
#pragma once

#include <cstdint>

namespace {

// C.  16 KiB: 1,024 units of 16 B, four to a thread of a workgroup of 256 (profiles/locate_seq_text.txt has the
// alternatives tried).
constexpr uint32_t kSeqTextChunk = 16384;
static_assert((kSeqTextChunk & (kSeqTextChunk - 1u)) == 0u && kSeqTextChunk % 16u == 0u, "a power of two, in 16-B units");

enum SeqPiece : uint32_t { SEQ_GT = 0, SEQ_RG, SEQ_NL_RG, SEQ_BASES, SEQ_NL_END, SEQ_PIECES };

constexpr uint64_t seq_plan_row_len(uint64_t rg_len, uint64_t n_bases) { return 1u + rg_len + 1u + n_bases + 1u; }

constexpr uint64_t seq_plan_chunks(uint64_t total) { return (total + kSeqTextChunk - 1u) / kSeqTextChunk; }
constexpr uint64_t seq_plan_chunk_begin(uint64_t k) { return k * kSeqTextChunk; }
constexpr uint64_t seq_plan_chunk_end(uint64_t k, uint64_t total) {
    return (k + 1u) * kSeqTextChunk < total ? (k + 1u) * kSeqTextChunk : total;
}

// The row that holds byte `pos` of the text, among rows [lo, hi): row_off[lo] <= pos < row_off[hi].  It is the last row
// that begins at or before pos; a row of zero bytes begins where its successor does, so it is never the last one and
// falls out of the search by itself.
template <typename U>
constexpr uint64_t seq_plan_row_at(const U *row_off, uint64_t lo, uint64_t hi, uint64_t pos) {
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (row_off[mid] <= pos)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// The row behind row r of rows [.., hi), where r ends at byte pos = row_off[r + 1] and pos < row_off[hi]: the next row
// that is not empty.  That is r + 1 unless lines without rows follow r; behind those, the search.
template <typename U>
constexpr uint64_t seq_plan_next_row(const U *row_off, uint64_t r, uint64_t hi, uint64_t pos) {
    return row_off[r + 2u] > pos ? r + 1u : seq_plan_row_at(row_off, r + 2u, hi, pos);
}

struct SeqRun {
    uint32_t piece;     // SeqPiece
    uint64_t src_off;   // first byte inside the piece
    uint64_t dst_off;   // first byte in the text
    uint64_t len;       // > 0
};

// The run that begins at byte `pos` of the text, inside the row that begins at row_off (row_off <= pos < row_off +
// seq_plan_row_len(rg_len, n_bases)), and ends with its piece or at `end` (> pos), whichever comes first.  rg_len and
// n_bases may be zero: an empty piece has no run.
constexpr SeqRun seq_plan_run(uint64_t row_off, uint64_t rg_len, uint64_t n_bases, uint64_t pos, uint64_t end) {
    const uint64_t d = pos - row_off;
    const uint64_t b_nl = 1u + rg_len, b_bases = b_nl + 1u, b_end = b_bases + n_bases;
    uint32_t piece = SEQ_NL_END;
    uint64_t first = b_end, last = b_end + 1u;           // the piece is bytes [first, last) of the row
    if (d == 0u)
        piece = SEQ_GT, first = 0u, last = 1u;
    else if (d < b_nl)
        piece = SEQ_RG, first = 1u, last = b_nl;
    else if (d == b_nl)
        piece = SEQ_NL_RG, first = b_nl, last = b_bases;
    else if (d < b_end)
        piece = SEQ_BASES, first = b_bases, last = b_end;
    const uint64_t in_piece = last - d, in_stretch = end - pos;
    return SeqRun{piece, d - first, pos, in_piece < in_stretch ? in_piece : in_stretch};
}

}  // namespace
