// The piece planner of csrc/vgl_pieces.h as a stand-alone host program (tests/test_sort_pieces_cpu.py builds and runs it).
// stdin: one case per line, "cap n k0 k1 ... k(n-1)".  stdout per case: "largest b0 b1 ... bm".
#include "../vectorgraphlibrary_amd/csrc/vgl_pieces.h"
#include <cstdio>

int main()
{
    long long cap = 0, n = 0;
    while (scanf("%lld %lld", &cap, &n) == 2) {
        std::vector<int64_t> keys((size_t)n), bounds;
        for (long long i = 0; i < n; i++) {
            long long k = 0;
            if (scanf("%lld", &k) != 1) return 1;
            keys[(size_t)i] = k;
        }
        const int64_t largest = vgl_plan_pieces((int64_t)n, [&](int64_t i) { return keys[(size_t)i]; }, (int64_t)cap, &bounds);
        printf("%lld", (long long)largest);
        for (int64_t b : bounds) printf(" %lld", (long long)b);
        printf("\n");
    }
    return 0;
}
