// Host-side unit test of the split pass's zero bound and class predicate
// (mpir-fft_amd/csrc/rdispatch.hpp: rp_zero_row, rp_live_slots, rp_pair_of, rp_class_single).
// The same functions run inside k_rpass MODE 2; they are __host__ __device__ so the CPU suite
// can pin them against a brute-force model of the DIF levels.
// Built by __graft_entry__.build() (tests/split_prune_host/Makefile), run by
// tests/test_split_prune_host.py.
#include "rdispatch.hpp"
#include <stdio.h>
#include <set>
#include <vector>

// Model: slot s starts with the set {s} if input s is live (s < nlive), else the empty set.  DIF
// level li pairs (i, k = i | 2^jb), jb = logg - 1 - li: both slots then hold the union.  Before
// each level, for every partner slot k: "single" iff its set has one element, and the
// representative is the lowest partner slot of the level with the same set.
static int check_classes(int logg)
{
    const int G = 1 << logg;
    int bad = 0;
    for (int nlive = 0; nlive <= G; ++nlive) {
        std::vector<std::set<int>> S(G);
        for (int s = 0; s < nlive; ++s) S[s].insert(s);
        for (int li = 0; li < logg; ++li) {
            const int jb = logg - 1 - li;
            for (int k = 0; k < G; ++k) {
                if (!(k >> jb & 1)) continue;
                const bool single = S[k].size() == 1;
                int rep = k;
                if (single)
                    for (int q = 0; q < G; ++q)
                        if ((q >> jb & 1) && S[q] == S[k]) { rep = q; break; }
                int got_rep = -1;
                const bool got = rp_class_single(logg, li, nlive, k, got_rep);
                if (got != single || got_rep != rep) {
                    if (bad++ < 8) printf("class mismatch G=%d li=%d nlive=%d k=%d: got %d rep %d want %d rep %d\n", G, li, nlive, k, (int)got, got_rep, (int)single, rep);
                }
                // the kernel's zero test: the class of k holds no live input iff its lowest member is dead
                const bool zero = S[k].empty(), kz = (k & ((1 << (logg - li)) - 1)) >= nlive;
                if (zero != kz) { if (bad++ < 8) printf("zero mismatch G=%d li=%d nlive=%d k=%d\n", G, li, nlive, k); }
                // the exchange slot of the representative is the pair it is the partner of, and a
                // published representative never collides with another published slot
                const int pi = rp_pair_of(logg, li, k);
                const int i = ((pi >> jb) << (jb + 1)) | (pi & ((1 << jb) - 1));
                if ((i | (1 << jb)) != k || pi < 0 || pi >= G / 2) { if (bad++ < 8) printf("pair mismatch G=%d li=%d k=%d pi=%d\n", G, li, k, pi); }
            }
            // copies: every slot of a single class must hold the same set (the model's stand-in for
            // "bit-for-bit copies": no butterfly with two non-zero inputs fed it)
            std::vector<std::set<int>> Nx = S;
            for (int pi = 0; pi < G / 2; ++pi) {
                const int i = ((pi >> jb) << (jb + 1)) | (pi & ((1 << jb) - 1)), k = i | (1 << jb);
                std::set<int> u = S[i];
                u.insert(S[k].begin(), S[k].end());
                Nx[i] = Nx[k] = u;
            }
            S = Nx;
        }
    }
    printf("G=%d classes bad=%d\n", G, bad);
    return bad;
}

static int check_bounds()
{
    int bad = 0;
    struct { long j, NC, cap, want; } c[] = {
        {1, 256, 156, 1},           // one coefficient: row 0 is live
        {256, 256, 156, 1},         // exactly one full row
        {257, 256, 156, 2},         // one coefficient past a row boundary: the partly filled row is live
        {19837, 256, 156, 78},      // C3: ceil(19837 / 256)
        {19968, 256, 156, 78},      // an exact multiple of NC
        {19969, 256, 156, 79},
        {40000, 256, 200, 157},     // j > n = 32768 (more than half of the NR = 256 rows)
        {65536, 256, 256, 256},     // every row
        {70000, 256, 256, 256},     // never past the cap
        {5, 1, 4, 4},
    };
    for (auto &t : c) {
        const long z = rp_zero_row(t.j, t.NC, t.cap);
        if (z != t.want) { if (bad++ < 8) printf("rp_zero_row(%ld, %ld, %ld) = %ld want %ld\n", t.j, t.NC, t.cap, z, t.want); }
    }
    // the bound against its definition: row r is live iff it holds a coefficient c < j, c / NC == r
    for (long NC : {1L, 2L, 8L, 16L})
        for (long NR : {2L, 8L, 32L})
            for (long j = 1; j <= NC * NR + 3; ++j) {
                long z = 0;
                for (long cidx = 0; cidx < j && cidx < NC * NR; ++cidx) z = cidx / NC + 1;
                if (rp_zero_row(j, NC, NR) != z) { if (bad++ < 8) printf("rp_zero_row(%ld, %ld, %ld) want %ld\n", j, NC, NR, z); }
            }
    // live slots of a group: positions pos0 + (i << lstep) below the bound, counted directly
    for (int logg = 1; logg <= 4; ++logg)
        for (int lstep = 0; lstep <= 4; ++lstep)
            for (int pos0 = 0; pos0 < (1 << lstep); ++pos0)
                for (int zf = 0; zf <= (1 << (logg + lstep)) + 2; ++zf) {
                    int n = 0;
                    for (int i = 0; i < (1 << logg); ++i) n += pos0 + (i << lstep) < zf;
                    if (rp_live_slots(1 << logg, pos0, lstep, zf) != n) { if (bad++ < 8) printf("rp_live_slots(%d, %d, %d, %d) want %d\n", 1 << logg, pos0, lstep, zf, n); }
                }
    printf("bounds bad=%d\n", bad);
    return bad;
}

int main()
{
    int bad = 0;
    for (int logg = 1; logg <= 4; ++logg) bad += check_classes(logg);   // G = 8 and 16 are the flagship groups
    bad += check_bounds();
    printf(bad ? "FAIL\n" : "OK\n");
    return bad ? 1 : 0;
}
