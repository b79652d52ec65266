// The pair state table's record index (common.h: pair_state_record) is a bijection onto [0, pair_state_records): checked on the
// host for every (trajectory, e, s, sn != s, sm != sn, t1, g1, q2) of small sets.  A wrong index is an out-of-bounds access of the
// builders or of begin_chain on the device; here it is a failed check, or a report of the sanitizer the program is built with:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I bild_amd/csrc \
//       tools/pair_state_index_check.cpp -o pair_state_index_check && ./pair_state_index_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "common.h"

using namespace bild;

namespace {

int check(int S, const std::vector<int> &Ts, int dstar_max, int G, int pnq)
{
    // the bases as bild_trajset_create lays them out: (S - 1)^2 entries for every prefix record of the trajectories in front
    std::vector<int64_t> base;
    int64_t prefix_records = 0;
    for (int T : Ts) {
        base.push_back(prefix_records * (S - 1) * (S - 1));
        prefix_records += (int64_t)T * S * dstar_max;
    }
    const int64_t records = pair_state_records(prefix_records, S, G, pnq);
    std::vector<unsigned char> seen((size_t)records, 0);
    int64_t hit = 0;
    for (size_t j = 0; j < Ts.size(); ++j)
        for (int e = 0; e < dstar_max; ++e)
            for (int s = 0; s < S; ++s)
                for (int sn = 0; sn < S; ++sn)
                    for (int sm = 0; sm < S; ++sm) {
                        if (sn == s || sm == sn) continue;
                        for (int t1 = 0; t1 < Ts[j]; ++t1)
                            for (int g1 = 1; g1 < G; ++g1)
                                for (int q2 = 0; q2 < pnq; ++q2) {
                                    const int64_t i = pair_state_record(base[j], S, Ts[j], G, pnq, e, s, sn, sm, t1, g1, q2);
                                    if (i < 0 || i >= records) {
                                        std::printf("S=%d T=%d G=%d pnq=%d: index %lld outside [0, %lld)\n", S, Ts[j], G, pnq, (long long)i, (long long)records);
                                        return 1;
                                    }
                                    if (seen[(size_t)i]++) {
                                        std::printf("S=%d T=%d G=%d pnq=%d: index %lld taken twice\n", S, Ts[j], G, pnq, (long long)i);
                                        return 1;
                                    }
                                    ++hit;
                                }
                    }
    if (hit != records) {
        std::printf("S=%d G=%d pnq=%d: %lld indices for %lld records\n", S, G, pnq, (long long)hit, (long long)records);
        return 1;
    }
    return 0;
}

} // namespace

int main()
{
    int bad = 0, cases = 0;
    for (int S : {2, 3})
        for (int dstar_max : {1, 2})
            for (int G : {2, 5, 46})
                for (int pnq : {1, 4, 15}) {
                    for (int T : {7, 50}) {
                        bad += check(S, {T}, dstar_max, G, pnq);
                        ++cases;
                    }
                    bad += check(S, {7, 50, 13}, dstar_max, G, pnq); // three trajectories of different lengths: the bases
                    ++cases;
                }
    std::printf("%d cases, %d failed\n", cases, bad);
    return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
