// vgl_pieces.h -- pieces of consecutive rows under a key cap: the host-side plan of the piecewise key sorts (simple.hip, quotient.hip).  Includes
// nothing of HIP, so a plain host compiler can build it.  DESIGN section 26.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

// Rows 0 .. n - 1, row i with keys(i) >= 0 keys, are cut greedily: a piece is closed before a row that would lift it above cap_keys, so a row with
// more keys than the cap is a piece of its own.  bounds = {0, ..., n}: piece k holds the rows [bounds[k], bounds[k + 1]); no piece is empty but the one
// of n == 0.  Returns the keys of the largest piece (0 when there are none: a caller that needs a buffer lifts that to 1).
template <class KEYS>
int64_t vgl_plan_pieces(int64_t n, KEYS keys, int64_t cap_keys, std::vector<int64_t> *bounds)
{
    bounds->assign(1, 0);
    int64_t acc = 0, largest = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t k = keys(i);
        if (acc > 0 && k > cap_keys - acc) { bounds->push_back(i); largest = std::max(largest, acc); acc = 0; }      // (acc + k > cap_keys, without overflow)
        acc += k;
    }
    bounds->push_back(n);
    return std::max(largest, acc);
}
