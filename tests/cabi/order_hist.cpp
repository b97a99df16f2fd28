// Drives gorder_amd/csrc/order_hist.h — the bin search k_bonds_dist and gorder_hip_set_order_histogram share — and
// choose_order_route of order_route.h with OrderRouteIn::dist set, without a device (built plainly and with
// -fsanitize=address,undefined by tests/test_order_histogram_cpu.py; tests/cabi/order_route.cpp never sets dist).
//
//   order_hist bins FILE   FILE holds ascending int32 edges, one per line.  Prints `tick bin` for every edge, every edge - 1 and
//                          + 1, -500000, 1000000, 0, the int32 limits and 1000 below the first and above the last edge.  The
//                          edges live in a heap block of their exact size: a read past them is the sanitizer's to find.
//   order_hist check       one line `case: ok` or `case: reason` per edge set of hist_edges_check
//   order_hist route       one line per input: the input's number i, then
//                          family label npf mom speculative extras items_by_slot ua_mode direct | family of the same facts without dist
//   Input i: bit k of i is the k-th of: bond_tiles, acos, use_gather, leaflets, global_leaflets, spec_enabled, have_assignment,
//   every_frame_assigns, pbc, geom, npf5, item_run; bits 12-13: axis - 1 ... the facts a handle with a histogram can have.
//   order_hist chunks      `n_frames n_tiles wg_target table_words samples_per_word -> frames_per_chunk n_chunks` for a few launches
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "order_hist.h"
#include "order_route.h"

using namespace gorder;

static int bins(const char *path) {
    std::FILE *f = std::fopen(path, "r");
    if (!f) return 2;
    std::vector<int32_t> read;
    long long v;
    while (std::fscanf(f, "%lld", &v) == 1) read.push_back((int32_t)v);
    std::fclose(f);
    int32_t *edges = new int32_t[read.size()];
    std::memcpy(edges, read.data(), read.size() * sizeof(int32_t));
    const uint32_t n = (uint32_t)read.size();
    if (hist_edges_check(edges, n)) { delete[] edges; return 3; }
    std::set<long long> ticks = {-500000, 1000000, 0, INT32_MIN, INT32_MAX, (long long)edges[0] - 1000, (long long)edges[n - 1] + 1000};
    for (uint32_t k = 0; k < n; k++)
        for (long long d = -1; d <= 1; d++) ticks.insert((long long)edges[k] + d);
    for (long long t : ticks)
        if (t >= INT32_MIN && t <= INT32_MAX) std::printf("%lld %d\n", t, hist_bin(edges, n, (int32_t)t));
    delete[] edges;
    return 0;
}

static void check_case(const char *name, const std::vector<int32_t> &e) {
    int32_t *edges = e.empty() ? nullptr : new int32_t[e.size()];
    if (edges) std::memcpy(edges, e.data(), e.size() * sizeof(int32_t));
    const char *why = hist_edges_check(edges, (uint32_t)e.size());
    std::printf("%s: %s\n", name, why ? why : "ok");
    delete[] edges;
}

static int check() {
    auto ramp = [](int n) { std::vector<int32_t> e; for (int k = 0; k < n; k++) e.push_back(-500000 + 3 * k); return e; };
    check_case("two", {-500000, 1000001});
    check_case("257", ramp(257));
    check_case("one", {0});
    check_case("none", {});
    check_case("258", ramp(258));
    check_case("equal", {0, 5, 5, 9});
    check_case("descending", {0, 5, 4, 9});
    check_case("limits", {INT32_MIN, 0, INT32_MAX});
    std::printf("null: %s\n", hist_edges_check(nullptr, 3) ? hist_edges_check(nullptr, 3) : "ok");
    return 0;
}

static int route() {
    for (uint32_t i = 0; i < (1u << 14); i++) {
        OrderRouteIn in;
        uint32_t k = 0;
        auto bit = [&]() { return ((i >> k++) & 1u) != 0; };
        in.bond_tiles = bit(); in.acos = bit(); in.use_gather = bit(); in.leaflets = bit(); in.global_leaflets = bit();
        in.spec_enabled = bit(); in.have_assignment = bit(); in.every_frame_assigns = bit(); in.pbc = bit();
        in.geom = bit();
        in.npf5 = bit(); in.item_run = bit();
        in.axis = (int)((i >> 12) & 3u) - 1;
        in.max_window = 340u;
        OrderRouteIn plain = in;
        in.dist = true;
        const OrderRoute r = choose_order_route(in), q = choose_order_route(plain);
        std::printf("%u %d %s %d %d %d %d %d %d %d | %d\n", i, (int)r.family, r.label ? r.label : "-", r.npf, (int)r.mom, (int)r.speculative,
                    (int)r.extras, (int)r.items_by_slot, r.ua_mode, (int)r.direct, (int)q.family);
    }
    return 0;
}

static int chunks() {
    const uint32_t cases[][5] = {{4000, 64, 0, 11520, 8}, {4000, 132, 0, 1980, 8}, {4000, 64, 0, 0, 8}, {11, 3, 0, 11520, 8}, {11, 2, 1, 352, 8},
                                 {4000, 64, 1, 11520, 8}, {20000000, 1, 1, 64, 8}, {1, 1, 0, 16384, 8}, {4000, 64, 0, 11520, 0},
                                 {4000, 64, 0, 11520, 65536}};
    for (const auto &c : cases) {
        const FrameChunks got = dist_chunks(c[0], c[1], c[2], 2048, c[3], c[4], 1u << 23);
        std::printf("%u %u %u %u %u -> %u %u\n", c[0], c[1], c[2], c[3], c[4], got.frames_per_chunk, got.n_chunks);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "bins")) return bins(argv[2]);
    if (argc >= 2 && !std::strcmp(argv[1], "check")) return check();
    if (argc >= 2 && !std::strcmp(argv[1], "route")) return route();
    if (argc >= 2 && !std::strcmp(argv[1], "chunks")) return chunks();
    return 1;
}
