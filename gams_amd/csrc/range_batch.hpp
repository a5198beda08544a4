// range_batch.hpp -- the one front and back of the range batches: gams_gpu_range_gc_batch (sw.hip) and
// gams_gpu_range_dg_batch (dg.hip).  Both take the ranges of n_sel selected ctgs, refuse what does not lie inside its ctg,
// stage their columns in one page-locked block, launch one kernel between the handle's k0 / k1 and read one float a range
// back.  An entry E says only what is its own:
//   int  admit()                    its refusals between the null arguments and the empty selection
//   Cols inputs(Carver &, n)        the layout of its staged columns (pinned, and at the head of the device block)
//   void head(in)                   what it stages once (the ctg records, the table)
//   int  range(in, k, q)            the columns of range q of selected ctg k, known to lie inside the ctg; its refusals
//   int  ready()                    the seqset made readable for its kernel (gams_seqset_gcindex, gams_dg_seq_ready)
//   void launch(d, n, d_out)        its kernel on the compute stream, over the device columns
#pragma once

#include "common.hpp"

struct RangeBatch {
    gams_seqset_t *s;
    uint32_t n_sel;
    const uint32_t *ctg_index;
    const int32_t *chr_start;
    const uint64_t *range_off;
    const int32_t *range_start, *range_end;
    float *out;
    // "<who>: range 7 of selected ctg 2", the head of every refusal of one range
    std::string which(const std::string &who, uint32_t k, uint64_t q) const {
        return who + ": range " + std::to_string(q - range_off[k]) + (n_sel > 1 ? " of selected ctg " + std::to_string(k) : std::string());
    }
};

template <typename E>
int gams_range_batch(gams_gpu_t *h, const std::string &who, const RangeBatch &b, E &&e) {
    gams_seqset_t *const s = b.s;
    const uint32_t n_sel = b.n_sel;
    if (!h || !s || (n_sel && (!b.ctg_index || !b.chr_start || !b.range_off))) return gams_fail(h, GAMS_EINVAL, who + ": null argument");
    int rc = e.admit();
    if (rc != GAMS_OK) return rc;
    if (n_sel == 0) return GAMS_OK;
    if ((rc = gams_sw_check_selection(h, who, "range_off", s, n_sel, b.ctg_index, b.range_off)) != GAMS_OK) return rc;
    const uint64_t n64 = b.range_off[n_sel];
    if (n64 == 0) return GAMS_OK;
    if (!b.range_start || !b.range_end || !b.out) return gams_fail(h, GAMS_EINVAL, who + ": null argument");
    if (n64 > 0x7fffff00ull) return gams_fail(h, GAMS_EUNSUPPORTED, who + ": too many ranges for one launch");
    const uint32_t n = (uint32_t)n64;
    GAMS_HIP(h, hipSetDevice(h->device));
    // inputs in one page-locked block (one DMA); results in the same device block
    auto inputs = [&](Carver &c) { return e.inputs(c, n); };
    const size_t in_bytes = layout_bytes(inputs);
    PoolBlock dev(h, false), pin(h, true);
    GAMS_TRY(h, who, pin.alloc(in_bytes));
    const auto in = carve(pin.p, inputs);
    e.head(in);
    for (uint32_t k = 0; k < n_sel; ++k) {
        const int32_t cs = b.chr_start[k];
        const int64_t ce = (int64_t)cs + s->len[b.ctg_index[k]] - 1;
        // (utils.rs:151-156 slices seq[from-1..to): a range outside the ctg, or inverted, panics there)
        for (uint64_t q = b.range_off[k]; q < b.range_off[k + 1]; ++q) {
            if (b.range_start[q] < cs || b.range_end[q] > ce || b.range_end[q] < b.range_start[q])
                return gams_fail(h, GAMS_EINVAL, b.which(who, k, q) + " is not inside the ctg");
            if ((rc = e.range(in, k, q)) != GAMS_OK) return rc;
        }
    }
    if ((rc = e.ready()) != GAMS_OK) return rc;
    auto d = in;   // (the same columns, carved off the device block below)
    float *d_out = nullptr;
    auto device = [&](Carver &c) {   // the inputs | results
        d = inputs(c);
        d_out = c.take<float>(n);
    };
    GAMS_TRY(h, who, dev.alloc(layout_bytes(device)));
    carve(dev.p, device);
    GAMS_TRY(h, who, hipMemcpyAsync(dev.p, pin.p, in_bytes, hipMemcpyHostToDevice, h->compute));
    GAMS_TRY(h, who, hipEventRecord(h->k0, h->compute));
    e.launch(d, n, d_out);
    GAMS_TRY(h, who, hipGetLastError());
    GAMS_TRY(h, who, hipEventRecord(h->k1, h->compute));
    h->k_valid = true;
    h->kq_used = 0;
    GAMS_TRY(h, who, hipMemcpyAsync(b.out, d_out, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->compute));
    GAMS_TRY(h, who, hipStreamSynchronize(h->compute));
    return GAMS_OK;
}
