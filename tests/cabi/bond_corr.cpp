// Drives gorder_amd/csrc/bond_corr.h — the lag check, the ring arithmetic, the chunks and the pair count that
// gorder_hip_set_bond_correlation and the submit path share — without a device (built plainly and with
// -fsanitize=address,undefined by tests/test_bond_correlation_cpu.py).
//
//   bond_corr check            one line `case: ok` or `case: reason` per lag list of corr_lags_check
//   bond_corr ring MAXLAG S [SHRINK]   a run of ragged batches cut into sub-ranges of S frames over a ring of corr_ring_planes(MAXLAG, S)
//                              planes: every sub-range writes its frames' planes, then every frame reads the planes of
//                              frame - lag for lag = 0 .. MAXLAG as far as the run reaches back.  The ring is a heap block of
//                              exactly R slots that hold the frame written last: prints `frames R reads` and exits 0 only if every
//                              read found the frame it asked for (SHRINK planes fewer than that: the same walk on a ring too small, which
//                              must exit 1)
//   bond_corr budget           `plane_bytes max_lag budget -> fit` for a few systems, then `fit batch forced -> subrange`
//   bond_corr chunks           `n_frames n_tiles wg_target -> frames_per_chunk n_chunks` for a few launches
//   bond_corr pairs            `frames lag samples -> pairs`
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bond_corr.h"

using namespace gorder;

static void check_case(const char *name, const std::vector<uint32_t> &l, bool null = false) {
    uint32_t *lags = l.empty() || null ? nullptr : new uint32_t[l.size()];      // exact size: a read past it is the sanitizer's to find
    if (lags) std::memcpy(lags, l.data(), l.size() * sizeof(uint32_t));
    const char *why = corr_lags_check(lags, (uint32_t)l.size());
    std::printf("%s: %s\n", name, why ? why : "ok");
    delete[] lags;
}

static int check() {
    auto ramp = [](uint32_t n, uint32_t step = 1) { std::vector<uint32_t> l; for (uint32_t k = 0; k < n; k++) l.push_back(k * step); return l; };
    check_case("none", {});
    check_case("one", {7});
    check_case("zero", {0});
    check_case("64", ramp(64, 65));
    check_case("65", ramp(65));
    check_case("equal", {0, 5, 5, 9});
    check_case("descending", {0, 5, 4, 9});
    check_case("4096", {0, 1, 4096});
    check_case("4097", {0, 1, 4097});
    check_case("only4097", {4097});
    check_case("null", {0, 1, 2}, true);
    return 0;
}

static int ring(uint32_t max_lag, uint32_t sub, uint32_t shrink) {
    const uint32_t R = corr_ring_planes(max_lag, sub) - shrink;
    int64_t *held = new int64_t[R];
    for (uint32_t k = 0; k < R; k++) held[k] = -1;
    const uint32_t batches[] = {1, 3, sub, 2 * sub + 1, 1, 1, max_lag + 5, 7, 3 * sub, 2, max_lag, 11};
    uint64_t seen = 0, reads = 0;
    int bad = 0;
    for (uint32_t nb : batches) {
        if (!nb) continue;
        for (uint32_t lo = 0; lo < nb; lo += sub) {
            const uint32_t hi = lo + sub < nb ? lo + sub : nb;
            for (uint32_t f = lo; f < hi; f++) held[corr_plane_of(seen + f, R)] = (int64_t)(seen + f);
            for (uint32_t f = lo; f < hi; f++)
                for (uint32_t lag = 0; lag <= max_lag && lag <= seen + f; lag++) {
                    reads++;
                    if (held[corr_plane_of(seen + f - lag, R)] != (int64_t)(seen + f - lag)) bad = 1;
                }
        }
        seen += nb;
    }
    delete[] held;
    std::printf("%llu %u %llu\n", (unsigned long long)seen, R, (unsigned long long)reads);
    return bad;
}

static int budget() {
    const uint64_t cases[][3] = {{262144, 4096, kCorrRingBudget}, {262144, 0, kCorrRingBudget}, {540672, 4096, kCorrRingBudget},
                                 {540672, 3970, kCorrRingBudget}, {14680064, 130, kCorrRingBudget}, {14680064, 146, kCorrRingBudget},
                                 {4096, 4096, kCorrRingBudget}, {0, 5, kCorrRingBudget}, {4096, 4, 4096u * 5u}, {4096, 5, 4096u * 5u}};
    for (const auto &c : cases)
        std::printf("%llu %llu %llu -> %llu\n", (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2],
                    (unsigned long long)corr_subrange_fit(c[0], (uint32_t)c[1], c[2]));
    const uint64_t subs[][3] = {{4096, 13, 0}, {4096, 13, 3}, {4096, 4000, 0}, {100, 4000, 0}, {100, 4000, 500}, {1, 1, 0}, {10, 1, 0}, {5000, 1, 1}};
    for (const auto &c : subs)
        std::printf("sub %llu %llu %llu -> %u\n", (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2],
                    corr_subrange(c[0], (uint32_t)c[1], (uint32_t)c[2]));
    return 0;
}

static int chunks() {
    const uint32_t cases[][3] = {{4000, 64, 0}, {4000, 132, 0}, {4000, 64, 1}, {13, 3, 0}, {13, 2, 1}, {1, 1, 0}, {100000, 1, 1}, {100000, 4, 0}, {64, 64, 0}, {65, 64, 0}};
    for (const auto &c : cases) {
        const CorrChunks got = corr_chunks(c[0], c[1], c[2], 2048);
        std::printf("%u %u %u -> %u %u\n", c[0], c[1], c[2], got.frames_per_chunk, got.n_chunks);
    }
    return 0;
}

static int pairs() {
    const uint64_t cases[][3] = {{13, 0, 40}, {13, 12, 40}, {13, 13, 40}, {13, 20, 40}, {0, 0, 40}, {4000, 2048, 256}, {1ull << 40, 4096, 1ull << 20}};
    for (const auto &c : cases)
        std::printf("%llu %llu %llu -> %llu\n", (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2],
                    (unsigned long long)corr_pair_count(c[0], (uint32_t)c[1], c[2]));
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "check")) return check();
    if (argc >= 4 && !std::strcmp(argv[1], "ring")) return ring((uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]), argc >= 5 ? (uint32_t)std::atoi(argv[4]) : 0u);
    if (argc >= 2 && !std::strcmp(argv[1], "budget")) return budget();
    if (argc >= 2 && !std::strcmp(argv[1], "chunks")) return chunks();
    if (argc >= 2 && !std::strcmp(argv[1], "pairs")) return pairs();
    return 1;
}
