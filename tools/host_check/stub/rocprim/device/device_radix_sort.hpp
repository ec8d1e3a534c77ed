// Stand-in for rocPRIM's pairs sort in tools/host_check/drivers_check.cpp: the size query answers with a size that follows the
// key width, the sort itself only records that it ran and with what.
#pragma once
#include <cstddef>
#include <vector>
#include <hip/hip_runtime.h>

namespace host_check {
struct SortCall {
    size_t bytes, n;
    unsigned end_bit;
};
extern int size_queries;
extern std::vector<SortCall> sorts;
void note(const char *what);
} // namespace host_check

namespace rocprim {
template <typename K, typename V>
hipError_t radix_sort_pairs(void *tmp, size_t &bytes, K *, K *, V *, V *, size_t n, unsigned, unsigned end_bit, hipStream_t) {
    if (tmp == nullptr) {
        bytes = 64 * (size_t)end_bit + n;
        ++host_check::size_queries;
        return hipSuccess;
    }
    host_check::sorts.push_back({bytes, n, end_bit});
    host_check::note("sort");
    return hipSuccess;
}
} // namespace rocprim
