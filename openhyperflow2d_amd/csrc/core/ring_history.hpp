// The rows a recorder's ring still holds, oldest first: the one reader of every
// per-step history (probes, loads, wall heat, surface) on both backends.
#pragma once

#include <algorithm>
#include <vector>

namespace hf2d {

// rows: [cap][row], times: [cap]; sample number q went to slot q % cap, and
// `total` samples were taken.  rows_out / times_out take the min(total, cap)
// kept samples in the order they were taken (cap == 0: none); time_of(t) is the
// reader's clock for a stored time.
template <class T, class TimeOf>
inline void ring_oldest_first(const T* rows, size_t row, const double* times, long total, long cap, TimeOf time_of,
                              std::vector<T>& rows_out, std::vector<double>& times_out) {
  const long n = cap ? std::min(total, cap) : 0, first = cap && total > cap ? total % cap : 0;
  times_out.resize(n);
  rows_out.resize((size_t)n * row);
  for (long k = 0; k < n; k++) {
    const long s = (first + k) % cap;
    times_out[k] = time_of(times[s]);
    std::copy(rows + (size_t)s * row, rows + (size_t)(s + 1) * row, rows_out.begin() + (size_t)k * row);
  }
}

}  // namespace hf2d
