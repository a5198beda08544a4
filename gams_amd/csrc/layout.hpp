// layout.hpp -- how a call lays its fields out in one pooled block: 256-B aligned slots, written once.
// Plain C++17 (no HIP): tests/layout_main.cpp checks the layouts below on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>

inline size_t gams_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Carves fields off a block.  A layout is a function over a Carver that fills a struct of typed pointers: run it over a
// null base to size the block (bytes()), then over the block -- once per block where a pinned and a device block share
// the layout.  take<T>(0) takes no bytes: a field that needs a slot of its own even when empty asks for max(n, 1).
struct Carver {
    uint8_t *base;
    size_t off = 0;
    explicit Carver(void *block = nullptr) : base(static_cast<uint8_t *>(block)) {}
    template <typename T>
    T *take(size_t count) { return reinterpret_cast<T *>(step(gams_align256(count * sizeof(T)))); }
    // no padding behind the field: the next one begins (or the block ends) where this one does
    template <typename T>
    T *take_tight(size_t count) { return reinterpret_cast<T *>(step(count * sizeof(T))); }
    uint8_t *step(size_t b) {
        uint8_t *const q = base ? base + off : nullptr;
        off += b;
        return q;
    }
    size_t bytes() const { return off; }
};

// layout = a callable over Carver &: the bytes it takes, and its pointers inside `block`
template <typename F>
size_t layout_bytes(F layout) {
    Carver c;
    (void)layout(c);
    return c.bytes();
}
template <typename F>
auto carve(void *block, F layout) {
    Carver c(block);
    return layout(c);
}

// ---- sw.hip: the inputs of gams_gpu_sw_batch and (without the row offsets) gams_gpu_range_gc_batch, pinned and device
template <typename Ctg>
struct SwStage {
    Ctg *ctgs;
    int32_t *fs, *fe;
    uint32_t *fctg;
    uint64_t *row_off;
};
template <typename Ctg>
SwStage<Ctg> sw_stage_layout(Carver &c, size_t n_sel, size_t nf, bool row_offsets) {
    SwStage<Ctg> s{};
    s.ctgs = c.take<Ctg>(n_sel);
    s.fs = c.take<int32_t>(nf);
    s.fe = c.take<int32_t>(nf);
    s.fctg = c.take<uint32_t>(nf);
    s.row_off = row_offsets ? c.take<uint64_t>(nf + 1) : nullptr;
    return s;
}

// ---- sw.hip: what the text kernels read beside the rows (page-locked, and at the head of the device text block)
struct SwTextTabs {
    uint64_t *ctg_row_off;
    uint32_t *name_off, *id_off;
    char *names, *ids;
};
inline SwTextTabs sw_text_tabs_layout(Carver &c, size_t n_sel, size_t nf, size_t name_bytes, size_t id_bytes) {
    SwTextTabs t{};
    t.ctg_row_off = c.take<uint64_t>(n_sel + 1);
    t.name_off = c.take<uint32_t>(n_sel + 1);
    t.names = c.take<char>(name_bytes + 1);
    t.id_off = c.take<uint32_t>(nf + 1);
    t.ids = c.take<char>(id_bytes + 1);
    return t;
}

// ---- interval.hip: the arena of an index (gams_index); bk: bk_slots cells of a starts' and a stops' record each
template <typename Group, typename CGroup, typename Rec, typename Bk>
struct IndexArena {
    Group *groups;
    CGroup *cgroups;
    uint32_t *stops, *lstart, *dir_start;
    Rec *lrec;
    Bk *bk;
};
template <typename Group, typename CGroup, typename Rec, typename Bk>
IndexArena<Group, CGroup, Rec, Bk> index_arena_layout(Carver &c, size_t n_groups, size_t m, size_t bk_slots) {
    const size_t ng1 = n_groups ? n_groups : 1, m1 = m ? m : 1;
    IndexArena<Group, CGroup, Rec, Bk> a{};
    a.groups = c.take<Group>(ng1);
    a.cgroups = c.take<CGroup>(ng1);
    a.stops = c.take<uint32_t>(m1);
    a.lstart = c.take<uint32_t>(m1);
    a.lrec = c.take<Rec>(m1);
    a.dir_start = c.take<uint32_t>(m + n_groups + 1);
    a.bk = c.take<Bk>(bk_slots);
    (void)c.take<Bk>(bk_slots);
    return a;
}

// ---- interval.hip: the scratch of one index build: raw columns, packed keys in / out, permutation in / out, offsets
struct IndexScratch {
    uint32_t *starts_in, *stops_in, *val_in, *val_out, *off32;
    uint64_t *key_in, *key_out;
};
inline IndexScratch index_scratch_layout(Carver &c, size_t n_groups, size_t m) {
    const size_t m1 = m ? m : 1;
    IndexScratch s{};
    s.starts_in = c.take<uint32_t>(m1);
    s.stops_in = c.take<uint32_t>(m1);
    s.key_in = c.take<uint64_t>(m1);
    s.key_out = c.take<uint64_t>(m1);
    s.val_in = c.take<uint32_t>(m1);
    s.val_out = c.take<uint32_t>(m1);
    s.off32 = c.take<uint32_t>(n_groups + 1);
    return s;
}

// ---- text.hip: the per-line columns of a text entry; n_rgg (count), n_cpos and prefix_len (anno) are 0 elsewhere
struct TextCols {
    unsigned long long *starts, *fend, *blk_bytes, *blk_off;   // fend: anno's prop
    uint32_t *grp, *qs, *qe, *cg, *cnt, *rgg;   // cg: count's rg group, anno's clip lo; cnt: count's counts, anno's clip hi
    int64_t *hit;
    uint8_t *keep;
    int32_t *cs, *ce;
    char *prefix;
};
inline TextCols text_cols_layout(Carver &c, size_t nl, size_t L, size_t nbr, size_t n_rgg, size_t n_cpos, size_t prefix_len) {
    TextCols t{};
    t.starts = c.take<unsigned long long>(nl + 2);
    t.grp = c.take<uint32_t>(L);
    t.qs = c.take<uint32_t>(L);
    t.qe = c.take<uint32_t>(L);
    t.cg = c.take<uint32_t>(L);
    t.cnt = c.take<uint32_t>(L);
    t.fend = c.take<unsigned long long>(L);
    t.hit = c.take<int64_t>(L);
    t.keep = c.take<uint8_t>(L);
    t.blk_bytes = c.take<unsigned long long>(nbr + 1);
    t.blk_off = c.take<unsigned long long>(nbr + 1);
    t.rgg = c.take<uint32_t>(n_rgg);
    t.cs = c.take<int32_t>(n_cpos);
    t.ce = c.take<int32_t>(n_cpos);
    t.prefix = c.take<char>(prefix_len + 1);
    return t;
}
