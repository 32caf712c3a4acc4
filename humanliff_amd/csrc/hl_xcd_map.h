// Block id -> work item for kernels whose workgroups share read-only data in groups (the attention: all query tiles of one (image, head) read
// the same K and V).  The dispatcher places workgroup b of a 1-D grid on XCD b % 8 (observed, speed only - nothing may depend on it): block b takes
// work item xcd * (total / 8) + min(xcd, total % 8) + b / 8, so every XCD gets one contiguous run of work items, and with the inner index fastest a
// contiguous run of groups in its L2.  Plain C++ as well as device code: tests/test_attention_map_cpu.py compiles this header on the host.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HL_XCD_MAP_FN __host__ __device__ inline
#else
#define HL_XCD_MAP_FN inline
#endif

namespace hl {

// work item of block b in a grid of `total` blocks: a bijection of [0, total)
HL_XCD_MAP_FN int xcd_work_item(int b, int total) {
    const int xcd = b & 7, slot = b >> 3;
    const int q8 = total >> 3, r8 = total & 7;
    return xcd * q8 + (xcd < r8 ? xcd : r8) + slot;
}

// ... split into (group, inner) with `inner_count` inner items per group, inner fastest.  place = false: block b is work item b (launch order: the groups'
// items go round the XCDs) - for grids of less than a workgroup per CU, which were measured faster with a group's readers spread over all eight L2s.
HL_XCD_MAP_FN void xcd_group_item(int b, int total, int inner_count, bool place, int &group, int &inner) {
    const int wi = place ? xcd_work_item(b, total) : b;
    group = wi / inner_count;
    inner = wi - group * inner_count;
}

}   // namespace hl
