// Drives gorder_amd/csrc/neighbour_classes.h — what gorder_hip_set_neighbour_classes and the launch code share — without a
// device (built plainly and with -fsanitize=address,undefined by tests/test_neighbour_classes_cpu.py).
//
//   neighbour_classes check      one line `case: ok` or `case: reason` per argument set of neighbour_args_check.  The index
//                                arrays live in heap blocks of their exact size: a read past them is the sanitizer's to find.
//   neighbour_classes pieces     `n -> n_pieces: len len ...` for list lengths around the piece size and the ABI's limit
//   neighbour_classes table      `planes n_classes slots -> bytes fits` around the 64-KB edge
//   neighbour_classes subrange   `n_frames n_mol forced row_bytes -> frames whole` for a few batches: the frames of a sub-range and
//                                whether the class rows hold the whole batch
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "neighbour_classes.h"

using namespace gorder;

static uint32_t *heap(const std::vector<uint32_t> &v) {
    if (v.empty()) return nullptr;
    uint32_t *p = new uint32_t[v.size()];
    std::memcpy(p, v.data(), v.size() * sizeof(uint32_t));
    return p;
}

static void check_case(const char *name, const std::vector<uint32_t> &centres, const std::vector<uint32_t> &neighbours, float radius,
                       uint32_t n_classes, uint32_t n_atoms, bool null_centres = false) {
    uint32_t *c = null_centres ? nullptr : heap(centres), *q = heap(neighbours);
    const char *why = neighbour_args_check(c, (uint32_t)centres.size(), q, (uint32_t)neighbours.size(), radius, n_classes, n_atoms);
    std::printf("%s: %s\n", name, why ? why : "ok");
    delete[] c;
    delete[] q;
}

static int check() {
    auto ramp = [](uint32_t n, uint32_t step = 1) { std::vector<uint32_t> v; for (uint32_t k = 0; k < n; k++) v.push_back(k * step); return v; };
    const uint32_t n_atoms = 20000;
    const std::vector<uint32_t> centres = ramp(40, 12);
    check_case("plain", centres, {1, 13, 25}, 1.0f, 4, n_atoms);
    check_case("one neighbour", centres, {19999}, 1.0f, 2, n_atoms);
    check_case("most neighbours", centres, ramp(kNeighbourMaxAtoms), 1.0f, kNeighbourMaxClasses, n_atoms);
    check_case("too many neighbours", centres, ramp(kNeighbourMaxAtoms + 1), 1.0f, 4, n_atoms);
    check_case("one class", centres, {1, 13}, 1.0f, 1, n_atoms);
    check_case("no class", centres, {1, 13}, 1.0f, 0, n_atoms);
    check_case("two classes", centres, {1, 13}, 1.0f, 2, n_atoms);
    check_case("most classes", centres, {1, 13}, 1.0f, kNeighbourMaxClasses, n_atoms);
    check_case("too many classes", centres, {1, 13}, 1.0f, kNeighbourMaxClasses + 1, n_atoms);
    check_case("radius zero", centres, {1, 13}, 0.0f, 4, n_atoms);
    check_case("radius negative", centres, {1, 13}, -1.0f, 4, n_atoms);
    check_case("radius nan", centres, {1, 13}, std::nanf(""), 4, n_atoms);
    check_case("radius inf", centres, {1, 13}, std::numeric_limits<float>::infinity(), 4, n_atoms);
    check_case("radius tiny", centres, {1, 13}, std::numeric_limits<float>::denorm_min(), 4, n_atoms);
    check_case("radius huge", centres, {1, 13}, std::numeric_limits<float>::max(), 4, n_atoms);
    check_case("centre last atom", {0, n_atoms - 1}, {1, 13}, 1.0f, 4, n_atoms);
    check_case("centre past the atoms", {0, n_atoms}, {1, 13}, 1.0f, 4, n_atoms);
    check_case("neighbour last atom", centres, {1, n_atoms - 1}, 1.0f, 4, n_atoms);
    check_case("neighbour past the atoms", centres, {1, n_atoms}, 1.0f, 4, n_atoms);
    check_case("equal", centres, {1, 13, 13}, 1.0f, 4, n_atoms);
    check_case("descending", centres, {1, 13, 12}, 1.0f, 4, n_atoms);
    check_case("null centres", centres, {1, 13}, 1.0f, 4, n_atoms, true);
    check_case("centres twice", {5, 5, 5}, {5}, 1.0f, 4, n_atoms);       // (allowed: two molecules may share a centre)
    return 0;
}

static int pieces() {
    for (uint32_t n : {0u, 1u, 1023u, 1024u, 1025u, 2048u, 2049u, 16383u, 16384u}) {
        std::printf("%u -> %u:", n, neighbour_pieces(n));
        for (uint32_t k = 0; k <= neighbour_pieces(n); k++) std::printf(" %u", neighbour_piece_len(n, k));     // (one past the last: 0)
        std::printf("\n");
    }
    return 0;
}

static int table() {
    const uint32_t cases[][3] = {{2, 32, 128}, {2, 32, 129}, {1, 32, 256}, {2, 32, 256}, {2, 16, 256}, {2, 17, 256}, {1, 2, 1}, {2, 8, 64}, {2, 8, 11},
                                 {2, 32, 0xffffffffu}};
    for (const auto &c : cases)
        std::printf("%u %u %u -> %llu %d\n", c[0], c[1], c[2], (unsigned long long)class_table_bytes(c[0], c[1], c[2]), (int)class_table_fits(c[0], c[1], c[2]));
    return 0;
}

static int subrange() {
    const uint64_t gib = kClassRowBytes;
    const uint64_t cases[][4] = {{4000, 3072, 0, gib}, {11, 40, 3, gib}, {11, 40, 0, gib}, {11, 40, 11, gib}, {11, 40, 12, gib}, {1, 1, 0, gib},
                                 {4000, 3072, 0, 3072 * 100}, {4000, 3072, 0, 3072 * 100 + 3071}, {4000, 3072, 0, 1}, {4000, 3072, 7, 3072 * 5},
                                 {0xffffffffull, 1, 0, gib}, {0xffffffffull, 0xffffffffull, 0, gib}, {100, 1u << 30, 0, gib}, {100, (1u << 30) + 1, 0, gib},
                                 {65534, 8, 0, gib}, {65535, 8, 0, gib}, {65536, 8, 0, gib}, {65600, 8, 0, gib}, {65600, 8, 70000, gib}, {65600, 8, 0, 8 * 70000},
                                 {200000, 16384, 0, gib}, {200000, 16385, 0, gib}};
    for (const auto &c : cases)
        std::printf("%llu %llu %llu %llu -> %u %d\n", (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3],
                    class_subrange((uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2], c[3]), (int)class_rows_whole((uint32_t)c[0], (uint32_t)c[1], c[3]));
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "check")) return check();
    if (argc >= 2 && !std::strcmp(argv[1], "pieces")) return pieces();
    if (argc >= 2 && !std::strcmp(argv[1], "table")) return table();
    if (argc >= 2 && !std::strcmp(argv[1], "subrange")) return subrange();
    return 1;
}
