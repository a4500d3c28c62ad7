// What the exact AUC's query passes share (the tree's and the distinct-key index's in
// auc_sort.hip, the count index's in count_query.hip): the workgroup size and the grid.
#pragma once

#include "dauc_internal.h"

namespace dauc {

constexpr int kQueryThreads = 1024;

inline int query_grid(int64_t L) {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
            (void)hipGetLastError();
            cus = 256;
        }
    }
    constexpr int qpt = 4;  // the queries per thread the grid aims at
    int64_t g = (L + int64_t(qpt) * kQueryThreads - 1) / (int64_t(qpt) * kQueryThreads);
    if (g > 1 * cus) g = 1 * cus;  // 1024-thread workgroups
    if (g < 1) g = 1;
    return static_cast<int>(g);
}

}  // namespace dauc
