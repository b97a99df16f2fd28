// The host decoder (xtc_reader.cpp) under AddressSanitizer / UBSan on the handcrafted streams of tests/xtc_streams.py:
// every file named on the command line is decoded frame by frame, whole and for the group of every third atom, and
// a checksum of the f32 bit patterns of each frame goes to stdout — "<file> <frame> <sum> <weighted sum>" twice over, or
// "<file> <frame> refused" — for tests/test_xtc_streams_cpu.py to compare with the reference decoder's.
// Built and run by that test (CPU only).
#include <cstdio>
#include <cstring>
#include <vector>
#include "gorder_xtc.h"

static void checksum(const std::vector<float> &x, unsigned long long &s1, unsigned long long &s2) {
    s1 = s2 = 0;
    for (size_t i = 0; i < x.size(); i++) {
        uint32_t u;
        memcpy(&u, &x[i], 4);
        s1 += u;
        s2 += (unsigned long long)(i + 1) * u;
    }
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        const char *path = argv[a];
        gorder_xtc_reader *whole = nullptr, *part = nullptr;
        if (gorder_xtc_open(path, nullptr, 0, &whole)) return 2;
        const uint32_t na = gorder_xtc_n_atoms_file(whole);
        std::vector<uint32_t> group;
        for (uint32_t i = 0; i < na; i += 3) group.push_back(i);
        if (gorder_xtc_open(path, group.data(), (uint32_t)group.size(), &part)) return 3;
        std::vector<float> x((size_t)na * 3), g(group.size() * 3), box(9);
        for (int frame = 0;; frame++) {
            const int st = gorder_xtc_next(whole, x.data(), box.data(), nullptr, nullptr, nullptr);
            const int sg = gorder_xtc_next(part, g.data(), box.data(), nullptr, nullptr, nullptr);
            if (st == GORDER_XTC_EOF && sg == GORDER_XTC_EOF) break;
            if (st == GORDER_XTC_ERR_FORMAT) {
                printf("%s %d refused\n", path, frame);
                continue;
            }
            if (st != GORDER_XTC_OK || sg != GORDER_XTC_OK) return 4;
            unsigned long long s1, s2, g1, g2;
            checksum(x, s1, s2);
            checksum(g, g1, g2);
            printf("%s %d %llu %llu %llu %llu\n", path, frame, s1, s2, g1, g2);
        }
        gorder_xtc_close(whole);
        gorder_xtc_close(part);
    }
    return 0;
}
