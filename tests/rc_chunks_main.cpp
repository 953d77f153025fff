// The chunk rule and mapping of csrc/vgl_chunks.h as a stand-alone host program (tests/test_rc_chunks_cpu.py builds and runs it).
// stdin: one case per line, "chunk_env longest nrows len0 ... len(nrows-1)"; the rows lie one after the other from entry 1000 on.
// stdout per case: "chunk nchunks", then per row "row_lo row_end k lo hi k lo hi ... split_ok" with the non-empty pieces in the order of k.
// split_ok: split(row * nchunks + k) gave (row, k) for every k that was looked at.  At most 4 pieces past the end of a row are looked at.
#include "../vectorgraphlibrary_amd/csrc/vgl_chunks.h"
#include <cstdio>

int main()
{
    long long env = 0, longest = 0, nrows = 0;
    while (scanf("%lld %lld %lld", &env, &longest, &nrows) == 3) {
        const vgl_rc_chunks ch = vgl_rc_chunks::of((int64_t)env, (int64_t)longest);
        printf("%d %d\n", (int)ch.chunk, (int)ch.nchunks);
        int64_t at = 1000;
        for (long long r = 0; r < nrows; r++) {
            long long len = 0;
            if (scanf("%lld", &len) != 1) return 1;
            const int64_t row_lo = at, row_end = at + (int64_t)len;
            at = row_end;
            printf("%lld %lld", (long long)row_lo, (long long)row_end);
            bool split_ok = true;
            int64_t empty = 0;
            for (int64_t k = 0; k < ch.nchunks && empty < 4; k++) {
                int64_t row = -1, kk = -1, lo = 0, hi = 0;
                ch.split((int64_t)r * ch.nchunks + k, &row, &kk);
                split_ok = split_ok && row == r && kk == k;
                if (ch.range(row_lo, row_end, k, &lo, &hi)) printf(" %lld %lld %lld", (long long)k, (long long)lo, (long long)hi);
                else empty++;
            }
            printf(" %d\n", split_ok ? 1 : 0);
        }
    }
    return 0;
}
