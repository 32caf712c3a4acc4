// Which tensor's GroupNorm totals may be trusted by whom (host bookkeeping of the UNet inference forward, hl_unet.cpp).
//
// A kernel that stores a tensor can add the tensor's fixed-point group totals into a statistics block (ConvArgs::stats, hl_stats.h).  A consumer
// may then form its GroupNorm coefficients from that block in-kernel (GnSrc), and the fp16x2 kernels take the activation scale sx of a raw
// input from it (ConvArgs::in_stats).  A block is handed to a consumer of tensor x only if
//   - exact cover: the block holds the totals of exactly x's channels - one producer of all of them at channel 0, or the two halves of a
//     decoder "concat" buffer, adjacent, both on ONE block.  A superset is refused - a record that covers more channels than x, or a part
//     that starts inside a wider view (c0 != 0): the rest of such a block belongs to a producer that nothing orders in front of x's consumer,
//     so the totals could still be growing and sx would depend on timing.  (totals_of tells a part by c0 and by the view's channel count: the
//     FIRST half of a concat asked for alone without need_view_match would pass.  The walk never reads a half alone.)
//   - ordering: every producer recorded for x was enqueued in front of the consumer on a stream the consumer is ordered behind (the walk
//     asks only when it enqueues a consumer of x, which is behind all of x's stores), so the totals are complete when the consumer runs.
// Whoever stored a tensor last owns its statistics: a store that leaves no totals (a skip convolution that the next launch finishes, a
// memcpy, a kernel without the statistics epilogue) withdraws what an earlier producer recorded.
//
// The book allocates nothing.  The walk hands every block in, in the same order in both of its passes: the sizing pass declares no concat,
// so every output there brings a block of its own - an upper bound of what the run pass, whose concat halves share one block, takes.
// Keys are the device addresses of channel 0 of the stored region and are never dereferenced.  Plain C++, no HIP: tests/test_stat_book_cpu.py
// compiles this header on the host.
#pragma once

#include <unordered_map>

namespace hl {

class StatBook {
  public:
    // where a producer adds: the block, the channels of the view the block's groups are formed for, the producer's first channel in that view
    struct Block { float *buf; int viewC, c0; };

    // the buffer at `cat` with C channels is normalised as ONE view: whoever stores [0, split) or [split, C) adds into `buf`
    void concat_halves(const float *cat, int C, int split, float *buf) {
        parts_[cat] = {buf, C, 0};
        parts_[cat + split] = {buf, C, split};
    }
    bool in_concat(const float *out) const { return parts_.count(out) != 0; }
    // the block an output of Cout channels at `out` adds into: the shared one of a declared concat half, else `fallback` as a view of its own
    Block block_for(const float *out, int Cout, float *fallback) const {
        auto f = parts_.find(out);
        return f != parts_.end() ? f->second : Block{fallback, Cout, 0};
    }

    // the tensor at p (`covered` channels) was stored with its totals added into b / without totals
    void produced(const float *p, const Block &b, int covered) { totals_[p] = {b, covered}; }
    void stored_without_totals(const float *p) { totals_.erase(p); }

    // the totals of the C-channel tensor at p under the rule above, whatever view they were grouped for or - need_view_match - only
    // those grouped for exactly this view (a GroupNorm over x); else null
    const float *totals_of(const float *p, int C, bool need_view_match) const {
        auto it = totals_.find(p);
        if (it == totals_.end() || it->second.b.c0 != 0 || (need_view_match && it->second.b.viewC != C)) return nullptr;
        const Entry &a = it->second;
        if (a.covered == C) return a.b.buf;
        auto it2 = totals_.find(p + a.covered);
        if (it2 != totals_.end() && it2->second.b.buf == a.b.buf && it2->second.b.c0 == a.covered && a.covered + it2->second.covered == C)
            return a.b.buf;
        return nullptr;
    }

  private:
    struct Entry { Block b; int covered; };
    std::unordered_map<const float *, Block> parts_;
    std::unordered_map<const float *, Entry> totals_;
};

}   // namespace hl
