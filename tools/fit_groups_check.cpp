// fit_groups_check.cpp - the fit launchers' query-group loop (csrc/sed_internal.h: sed_fit_each_query_group) on the host,
// with a recording callback in place of a launch: no device, no Python.  For nqueries = 0, 1, 65535, 65536, 131070, 131071
// and for nchunks = 0 it asserts that the groups tile [0, nqueries) in order, that none exceeds SED_FIT_MAX_QUERIES, that
// ev0 goes to the first group only and ev1 to the last only, and that a callback's error ends the loop and is returned.
// Build and run under the sanitizers, from the repository root:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ \
//         -I/opt/rocm/include -Irna-sequence-diff-patch_amd/csrc tools/fit_groups_check.cpp -o /tmp/fit_groups_check \
//         && /tmp/fit_groups_check
#include "sed_internal.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            fprintf(stderr, "%s:%d: %s (nqueries %d)\n", __FILE__, __LINE__, #cond, nqueries); \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

struct Group {
    int q0, nq;
    hipEvent_t e0, e1;
};

int main() {
    // (the helper only hands the events on: two distinct non-null values stand for them)
    static char tag[2];
    const hipEvent_t ev0 = (hipEvent_t)&tag[0], ev1 = (hipEvent_t)&tag[1];
    const int cases[] = {0, 1, 65535, 65536, 131070, 131071};
    for (int nqueries : cases) {
        std::vector<Group> got;
        const hipError_t e = sed_fit_each_query_group(1, nqueries, ev0, ev1, [&](int q0, int nq, hipEvent_t e0, hipEvent_t e1) {
            got.push_back(Group{q0, nq, e0, e1});
            return hipSuccess;
        });
        CHECK(e == hipSuccess);
        CHECK(got.size() == (size_t)((nqueries + SED_FIT_MAX_QUERIES - 1) / SED_FIT_MAX_QUERIES));
        int next = 0;
        for (size_t g = 0; g < got.size(); ++g) {
            CHECK(got[g].q0 == next);
            CHECK(got[g].nq >= 1 && got[g].nq <= SED_FIT_MAX_QUERIES);
            CHECK(got[g].e0 == (g == 0 ? ev0 : nullptr));
            CHECK(got[g].e1 == (g + 1 == got.size() ? ev1 : nullptr));
            next += got[g].nq;
        }
        CHECK(next == nqueries);
        // no chunk record: nothing runs, whatever the queries
        int calls = 0;
        CHECK(sed_fit_each_query_group(0, nqueries, ev0, ev1, [&](int, int, hipEvent_t, hipEvent_t) {
                  ++calls;
                  return hipSuccess;
              }) == hipSuccess);
        CHECK(calls == 0);
        // an error of group `bad` ends the loop there and is what the helper returns
        for (size_t bad = 0; bad < got.size(); ++bad) {
            size_t seen = 0;
            const hipError_t eb = sed_fit_each_query_group(1, nqueries, ev0, ev1, [&](int, int, hipEvent_t, hipEvent_t) {
                return seen++ == bad ? hipErrorLaunchFailure : hipSuccess;
            });
            CHECK(eb == hipErrorLaunchFailure);
            CHECK(seen == bad + 1);
        }
    }
    printf("fit_groups_check ok\n");
    return 0;
}
