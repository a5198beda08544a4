// Stand-alone driver of gams_amd/csrc/layout.hpp for tests/test_layout_cpu.py: host compiler, no HIP, no device.
// stdin: one layout per line (its name, then its sizes).  stdout, per line: the name, the bytes of the sizing pass (null
// base), the bytes of the pointer pass, then one "offset,extent" per field in layout order -- offset from the pointer
// pass over a real block, extent = the bytes the field's users index (count * element size).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../gams_amd/csrc/layout.hpp"

// stand-ins with the sizes of the device records (sw.hip and interval_kernels.hpp assert theirs)
struct Ctg { char b[32]; };
struct Group { char b[80]; };
struct CGroup { char b[32]; };
struct Rec { char b[16]; };
struct Bk { char b[32]; };

struct Field {
    const void *p;
    size_t extent;
};

template <typename F>
static void report(const char *name, F layout) {
    std::vector<Field> fields;
    Carver sizing;
    layout(sizing, fields);
    for (const Field &f : fields)
        if (f.p) {
            std::printf("%s\tsizing pass returned a pointer\n", name);
            return;
        }
    const size_t bytes = sizing.bytes();
    uint8_t *block = static_cast<uint8_t *>(std::aligned_alloc(256, gams_align256(bytes ? bytes : 1)));
    std::memset(block, 0, bytes);
    fields.clear();
    Carver pointers(block);
    layout(pointers, fields);
    std::printf("%s\t%zu\t%zu", name, bytes, pointers.bytes());
    for (const Field &f : fields) {
        const uint8_t *q = static_cast<const uint8_t *>(f.p);
        if (f.extent) std::memset(const_cast<uint8_t *>(q), 0x5a, f.extent);      // inside the block, or the sanitizer says so
        std::printf("\t%zu,%zu", (size_t)(q - block), f.extent);
    }
    std::printf("\n");
    std::free(block);
}

int main() {
    char name[32];
    unsigned long long v[6];
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        std::memset(v, 0, sizeof v);
        if (std::sscanf(line, "%31s %llu %llu %llu %llu %llu %llu", name, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) < 1) continue;
        const std::string n = name;
        if (n == "sw" || n == "range_gc") {
            const size_t n_sel = v[0], nf = v[1];
            const bool offs = n == "sw";
            report(name, [&](Carver &c, std::vector<Field> &f) {
                const SwStage<Ctg> s = sw_stage_layout<Ctg>(c, n_sel, nf, offs);
                f = {{s.ctgs, n_sel * sizeof(Ctg)}, {s.fs, nf * 4}, {s.fe, nf * 4}, {s.fctg, nf * 4}};
                if (offs) f.push_back({s.row_off, (nf + 1) * 8});
            });
        } else if (n == "sw_tabs") {
            const size_t n_sel = v[0], nf = v[1], nb = v[2], ib = v[3];
            report(name, [&](Carver &c, std::vector<Field> &f) {
                const SwTextTabs t = sw_text_tabs_layout(c, n_sel, nf, nb, ib);
                f = {{t.ctg_row_off, (n_sel + 1) * 8}, {t.name_off, (n_sel + 1) * 4}, {t.names, nb}, {t.id_off, (nf + 1) * 4}, {t.ids, ib}};
            });
        } else if (n == "arena") {
            const size_t ng = v[0], m = v[1], bk_slots = (m >> 1) + 2 * ng + 2;
            report(name, [&](Carver &c, std::vector<Field> &f) {
                const auto a = index_arena_layout<Group, CGroup, Rec, Bk>(c, ng, m, bk_slots);
                f = {{a.groups, ng * sizeof(Group)}, {a.cgroups, ng * sizeof(CGroup)}, {a.stops, m * 4}, {a.lstart, m * 4},
                     {a.lrec, m * sizeof(Rec)}, {a.dir_start, (m + ng + 1) * 4}, {a.bk, 2 * bk_slots * sizeof(Bk)}};
            });
        } else if (n == "scratch") {
            const size_t ng = v[0], m = v[1];
            report(name, [&](Carver &c, std::vector<Field> &f) {
                const IndexScratch s = index_scratch_layout(c, ng, m);
                f = {{s.starts_in, m * 4}, {s.stops_in, m * 4}, {s.key_in, m * 8}, {s.key_out, m * 8},
                     {s.val_in, m * 4}, {s.val_out, m * 4}, {s.off32, (ng + 1) * 4}};
            });
        } else if (n == "text") {
            const size_t nl = v[0], L = v[1], nbr = v[2], n_rgg = v[3], n_cpos = v[4], pre = v[5];
            report(name, [&](Carver &c, std::vector<Field> &f) {
                const TextCols t = text_cols_layout(c, nl, L, nbr, n_rgg, n_cpos, pre);
                f = {{t.starts, (nl + 2) * 8}, {t.grp, L * 4}, {t.qs, L * 4}, {t.qe, L * 4}, {t.cg, L * 4}, {t.cnt, L * 4},
                     {t.fend, L * 8}, {t.hit, L * 8}, {t.keep, L}, {t.blk_bytes, (nbr + 1) * 8}, {t.blk_off, (nbr + 1) * 8},
                     {t.rgg, n_rgg * 4}, {t.cs, n_cpos * 4}, {t.ce, n_cpos * 4}, {t.prefix, pre + 1}};
            });
        } else if (n == "tight") {
            // take_tight leaves no padding: a (count v[0]) of 24-B records, then an aligned field, as sw.hip's device block
            const size_t rows = v[0], cnt = v[1];
            report(name, [&](Carver &c, std::vector<Field> &f) {
                struct Row { char b[24]; };
                const Row *r = c.take_tight<Row>(rows);
                const int32_t *k = c.take<int32_t>(cnt);
                f = {{r, rows * sizeof(Row)}, {k, cnt * 4}};
            });
        } else {
            std::printf("%s\tunknown layout\n", name);
        }
    }
    return 0;
}
