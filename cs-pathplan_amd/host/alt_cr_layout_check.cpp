// alt_cr_layout_check.cpp -- CPU check of the workspace regions of the cyclic-reduction altitude kernels
// (cs-pathplan_amd/csrc/alt_cr_layout.h).  For every problem length n in 1..NMAX, with the largest batch the
// cyclic-reduction path takes: the parts of a region (solution, block rows, active flags) lie in order inside it, a region
// ends where the next problem's begins at the latest, and the last region ends inside csp_alt_workspace_bytes(total).
// Two neighbours of different lengths are covered too: a region's end depends only on its own start and length.
// usage: alt_cr_layout_check NMAX   -> exit 0 / 1
#include <cstdio>
#include <cstdlib>

#include "../csrc/alt_cr_layout.h"

using csp::alt::CrRegion;

static bool check(int64_t nmax) {
    const int64_t B = csp::alt::CR_MAX_BATCH;
    for (int64_t n = 1; n <= nmax; ++n) {
        // B problems of n samples: regions back to back
        for (int64_t b = 0; b < B; ++b) {
            const CrRegion r = csp::alt::cr_region(b * n, b, n);
            const int64_t next = b + 1 < B ? csp::alt::cr_region((b + 1) * n, b + 1, 1).x
                                           : (int64_t)(csp::alt::workspace_bytes(B * n) / sizeof(double));
            if (!(r.x <= r.store && r.store <= r.act && r.act <= r.end)) {
                std::fprintf(stderr, "n = %lld, problem %lld: parts out of order\n", (long long)n, (long long)b);
                return false;
            }
            if (r.store - r.x < n || r.end - r.act < n) {
                std::fprintf(stderr, "n = %lld: the solution or the flags do not fit\n", (long long)n);
                return false;
            }
            if (r.end > next) {
                std::fprintf(stderr, "n = %lld, problem %lld of %lld: region ends at %lld, the next one (or the workspace) at %lld\n",
                             (long long)n, (long long)b, (long long)B, (long long)r.end, (long long)next);
                return false;
            }
        }
        // a problem of n samples ahead of a long one, and a long one ahead of it
        const int64_t m = 4097;
        const CrRegion a = csp::alt::cr_region(0, 0, n), c = csp::alt::cr_region(n, 1, m);
        if (a.end > c.x || c.end > (int64_t)(csp::alt::workspace_bytes(n + m) / sizeof(double))) {
            std::fprintf(stderr, "n = %lld ahead of %lld: overlap\n", (long long)n, (long long)m);
            return false;
        }
    }
    return true;
}

int main(int argc, char **argv) {
    const int64_t nmax = argc > 1 ? std::atoll(argv[1]) : 5000;
    if (!check(nmax)) return 1;
    std::printf("ok n = 1..%lld, %lld problems\n", (long long)nmax, (long long)csp::alt::CR_MAX_BATCH);
    return 0;
}
