// csa_waves.h -- how the archive layer sizes its work to the device's memory: the HBM budget of a call and the number of tasks in
// a wave.  Plain C++, no HIP: tests/model/csa_dev_model.cpp runs wave_count on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/csa_mi355x.h"

namespace csa {

// CSAOptions::hbm_budget, or 3/4 of the device memory that is free now
inline uint64_t hbm_budget(const CSAOptions &o, size_t mem_free)
{
    return o.hbm_budget ? o.hbm_budget : (uint64_t)mem_free / 4 * 3;
}

// The number of tasks in the wave that begins at task `first` of `n`: at most `width`, and as many as need(task) bytes each fit
// into `budget` together.  The first task is taken whatever it needs, so the result is at least 1 when first < n.  The sum
// saturates: a need of UINT64_MAX, or a sum that would wrap, fits no budget.
template <class Need>
size_t wave_count(size_t first, size_t n, size_t width, uint64_t budget, Need need)
{
    size_t count = 0;
    uint64_t mem = 0;
    while (first + count < n && (count < width || !count)) {
        uint64_t sum;
        if (__builtin_add_overflow(mem, (uint64_t)need(first + count), &sum)) sum = UINT64_MAX;
        if (count && (sum == UINT64_MAX || sum > budget)) break;
        mem = sum;
        count++;
    }
    return count;
}

}   // namespace csa
