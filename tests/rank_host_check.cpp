// rank_host_check.cpp — a stand-alone check of the host arithmetic of the rank and count queries (clip_cpp_amd/csrc/rank_host.h: the
// checks of target_lims and radii, the cut into blocks, the CSR expansion), built with -fsanitize=address,undefined and run on the CPU
// by tests/test_rank_host.py.  Every array is heap-allocated at its exact size, so a read or write past an end is reported.
#include <cmath>
#include <cstdlib>
#include <vector>

#include "rank_host.h"

using namespace clipamd::idx;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "rank_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

// every block of a call, expanded, against the plain definition: column c belongs to the query whose [lims[q], lims[q + 1]) holds it
static int walk(const std::vector<int64_t> & lims, int64_t block) {
    const int64_t nq = (int64_t)lims.size() - 1, ncols = lims.back();
    std::vector<int64_t> owner;
    for (int64_t q = 0; q < nq; q++) owner.insert(owner.end(), (size_t)(lims[q + 1] - lims[q]), q);
    int64_t c0 = 0, last_q = 0;
    while (c0 < ncols) {
        const RankBlock b = rank_block_at(nq, lims.data(), c0, block);
        CHECK(b.c0 == c0 && b.c1 > c0 && b.c1 <= ncols && b.c1 - b.c0 <= block);
        CHECK(b.q_lo >= last_q && b.q_hi > b.q_lo && b.q_hi <= nq && b.q_hi - b.q_lo <= block);
        std::vector<int> qof((size_t)(b.c1 - b.c0), -1);
        rank_expand(lims.data(), b, qof.data());
        for (int64_t c = b.c0; c < b.c1; c++) CHECK(qof[(size_t)(c - b.c0)] + b.q_lo == owner[(size_t)c]);
        last_q = b.q_lo;
        c0 = b.c1;
    }
    return 0;
}

int main() {
    // the checks
    const std::vector<int64_t> good = {0, 0, 3, 3, 10}, late = {1, 2, 3}, down = {0, 4, 3, 5};
    CHECK(check_rank_lims(4, good.data(), "t") && check_rank_lims(7, nullptr, "t") && check_rank_lims(0, good.data(), "t"));
    CHECK(!check_rank_lims(2, late.data(), "t") && !check_rank_lims(3, down.data(), "t"));
    CHECK(rank_columns(4, good.data()) == 10 && rank_columns(7, nullptr) == 7);
    const std::vector<float> radii = {0.f, -1.f, INFINITY, 4.f}, with_nan = {0.f, NAN};
    CHECK(check_radii(radii.data(), 4, "t") && !check_radii(with_nan.data(), 2, "t") && check_radii(nullptr, 0, "t"));
    // one target per query: blocks of whole queries
    for (int64_t c0 = 0; c0 < 10; c0 += 4) {
        const RankBlock b = rank_block_at(10, nullptr, c0, 4);
        CHECK(b.q_lo == c0 && b.c1 == std::min<int64_t>(10, c0 + 4) && b.q_hi == b.c1);
    }
    // CSR: empty queries at both ends and in runs longer than a block, a query longer than several blocks, seeded random shapes
    if (walk({0, 0, 0, 5, 5, 5, 5, 5, 5, 5, 6, 30, 30, 31, 31, 31}, 4)) return 1;
    if (walk(good, RANK_BLOCK)) return 1;
    srand(5);
    for (int t = 0; t < 200; t++) {
        std::vector<int64_t> lims = {0};
        for (int q = 0, nq = rand() % 40; q < nq; q++) lims.push_back(lims.back() + (rand() % 3 ? rand() % 4 : rand() % 25));
        if (walk(lims, 1 + rand() % 9)) return 1;
    }
    printf("rank_host_check ok\n");
    return 0;
}
