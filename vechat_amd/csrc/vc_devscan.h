// The hipcub calls of the overlapper, the scrubber and the clusterer: the stable radix sort of pairs over a bit range and the two prefix sums.
// Each queries the size of the temporary storage, takes it from the caller's DevMem, runs on the null stream, waits and drops it.
// Nothing is cached between calls.
#pragma once

#include <hipcub/hipcub.hpp>

#include "vc_devutil.h"

namespace vc_dev {

// The envelope of every caller: fewer than 2^31 items (VC_OVL_MAX_SEQS, VC_OVL_MAX_LEN and the "2^31 entries per call" checks of
// the overlapper, "2 m < 2^31" of the scrubber).  It is checked here, once; a count beyond it fails like any other error.
inline bool in_envelope(uint64_t n) { return n < (1ull << 31); }

// stable, by the bits [0, bits) of the key.  The count goes to hipcub in 32 bits: below 2^31 items the sort needs no wider offsets
template <class K, class V>
bool sort_pairs(DevMem& m, const K* ki, K* ko, const V* vi, V* vo, uint64_t n, int bits) {
    if (!in_envelope(n)) return false;
    size_t tb = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, tb, ki, ko, vi, vo, (uint32_t)n, 0, bits, (hipStream_t)0) != hipSuccess) return false;
    uint8_t* tmp = nullptr;
    if (!m.alloc(&tmp, tb)) return false;
    const bool ok = hipcub::DeviceRadixSort::SortPairs(tmp, tb, ki, ko, vi, vo, (uint32_t)n, 0, bits, (hipStream_t)0) == hipSuccess;
    (void)hipDeviceSynchronize();
    m.drop(tmp);
    return ok;
}

template <bool Inclusive, class T>
bool prefix_sum(DevMem& m, const T* in, T* out, uint64_t n) {
    if (!in_envelope(n)) return false;
    auto sum = [&](void* tmp, size_t& tb) {
        return Inclusive ? hipcub::DeviceScan::InclusiveSum(tmp, tb, in, out, n, (hipStream_t)0)
                         : hipcub::DeviceScan::ExclusiveSum(tmp, tb, in, out, n, (hipStream_t)0);
    };
    size_t tb = 0;
    if (sum(nullptr, tb) != hipSuccess) return false;
    uint8_t* tmp = nullptr;
    if (!m.alloc(&tmp, tb)) return false;
    const bool ok = sum(tmp, tb) == hipSuccess;
    (void)hipDeviceSynchronize();
    m.drop(tmp);
    return ok;
}
template <class T> bool inclusive_sum(DevMem& m, const T* in, T* out, uint64_t n) { return prefix_sum<true>(m, in, out, n); }
template <class T> bool exclusive_sum(DevMem& m, const T* in, T* out, uint64_t n) { return prefix_sum<false>(m, in, out, n); }

}  // namespace vc_dev
