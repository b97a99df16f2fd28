// The TRR side of the host packer (gorder_xtc_pack_window* on TRR readers, gorder_xtc_probe_format, gorder_xtc_read_at)
// under AddressSanitizer / UBSan, as a program of its own: it writes small TRR files (single and double precision; a
// frame with velocities only, a frame without a box, two files with a duplicated boundary frame; a file cut inside a
// positions block, a frame whose positions size disagrees with its atom count), packs them — synchronously and through
// the copy pool, whole and with groups, with blobs that hold two frames or none — and compares with
// gorder_xtc_read_window.  Built and run by tools/trr_pack_sanitize.sh (CPU only).  usage: trr_pack_sanitize <directory>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "gorder_xtc.h"

namespace {
constexpr uint32_t N = 37;
void put32(std::vector<uint8_t> &o, uint32_t v) { for (int s = 24; s >= 0; s -= 8) o.push_back((uint8_t)(v >> s)); }
void put_real(std::vector<uint8_t> &o, double v, bool dbl) {
    if (dbl) { uint64_t u; memcpy(&u, &v, 8); put32(o, (uint32_t)(u >> 32)); put32(o, (uint32_t)u); }
    else { const float f = (float)v; uint32_t u; memcpy(&u, &f, 4); put32(o, u); }
}
// one frame: positions (or velocities only), with or without a box; x_size: the positions size the header claims
void frame(std::vector<uint8_t> &o, int step, double t, bool box, bool positions, bool dbl, const float *x, long x_size = -1) {
    const uint32_t rs = dbl ? 8 : 4;
    put32(o, 1993); put32(o, 13); put32(o, 12);
    for (const char *c = "GMX_trn_file"; *c; c++) o.push_back((uint8_t)*c);
    const uint32_t sizes[10] = {0, 0, box ? 9 * rs : 0, 0, 0, 0, 0, positions ? (x_size >= 0 ? (uint32_t)x_size : 3 * N * rs) : 0,
                                positions ? 0 : 3 * N * rs, 0};
    for (uint32_t s : sizes) put32(o, s);
    put32(o, N); put32(o, (uint32_t)step); put32(o, 0);
    put_real(o, t, dbl); put_real(o, 0.0, dbl);
    if (box) for (int k = 0; k < 9; k++) put_real(o, k % 4 == 0 ? 5.0 + k : 0.0, dbl);
    for (uint32_t k = 0; k < 3 * N; k++) put_real(o, (double)x[k] + (dbl ? 1e-9 * k : 0.0), dbl);
}
bool write_file(const std::string &path, const std::vector<uint8_t> &bytes, size_t n) {
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) return false;
    const bool ok = fwrite(bytes.data(), 1, n, fp) == n;
    fclose(fp);
    return ok;
}
int fail(int code, const char *what) { printf("FAILED (%d): %s\n", code, what); return code; }

// pack `paths` as one trajectory in windows of 3 frames and compare with gorder_xtc_read_window
int compare(const std::vector<std::string> &paths, const std::vector<uint32_t> &group, float begin, float end, uint32_t step, bool dbl,
            bool pooled) {
    const uint32_t nout = group.empty() ? N : (uint32_t)group.size();
    std::vector<float> rx, rb, rt;
    uint64_t state = 0; double last = -INFINITY;
    for (const std::string &p : paths) {
        gorder_xtc_reader *r = nullptr;
        if (gorder_xtc_open(p.c_str(), group.empty() ? nullptr : group.data(), (uint32_t)group.size(), &r)) return 10;
        std::vector<float> x((size_t)4 * nout * 3), b(4 * 9), t(4);
        int64_t got;
        while ((got = gorder_xtc_read_window(r, begin, end, step, &state, &last, x.data(), b.data(), t.data(), 4)) > 0) {
            rx.insert(rx.end(), x.begin(), x.begin() + got * nout * 3);
            rb.insert(rb.end(), b.begin(), b.begin() + got * 9);
            rt.insert(rt.end(), t.begin(), t.begin() + got);
        }
        gorder_xtc_close(r);
        if (got < 0) return 11;
    }
    const uint64_t state_read = state; const double last_read = last;
    state = 0; last = -INFINITY;
    gorder_xtc_pool *pool = nullptr;
    if (pooled && gorder_xtc_pool_create(3, &pool)) return 12;
    size_t k = 0;
    int rc = 0;
    for (const std::string &p : paths) {
        gorder_xtc_reader *r = nullptr;
        if (gorder_xtc_open(p.c_str(), group.empty() ? nullptr : group.data(), (uint32_t)group.size(), &r)) return 13;
        if (gorder_xtc_can_pack(r) != 1 || gorder_xtc_is_xtc(r) != 0) rc = 14;
        const uint32_t n_stop = gorder_xtc_n_atoms_needed(r), rs = dbl ? 8 : 4;
        const size_t per_frame = (((size_t)n_stop * 3 * rs + 63) & ~(size_t)63) + 64, cap = 2 * per_frame + 17;   // two frames fit
        std::vector<uint8_t> blob(cap);
        std::vector<gorder_xtc_frame_t> fr(3);
        std::vector<float> b(3 * 9), t(3), one((size_t)nout * 3), ob(9);
        std::vector<int64_t> pos(3);
        for (int64_t got = 1; got > 0 && !rc;) {
            uint64_t used = 0;
            got = gorder_xtc_pack_window_ex(r, begin, end, step, &state, &last, blob.data(), cap, &used, fr.data(), b.data(), t.data(), 3,
                                            2, pool, 1000, pos.data());
            if (pool && got >= 0 && gorder_xtc_pool_wait(pool)) rc = 15;
            if (got < 0) rc = 16;
            if (got > 2) rc = 17;                                  // the blob holds two
            for (int64_t q = 0; q < got && !rc; q++, k++) {
                if (k >= rt.size() || t[q] != rt[k] || memcmp(&b[9 * q], &rb[9 * k], 36)) { rc = 18; break; }
                if (fr[q].offset % 64 || fr[q].kind != (dbl ? 8u : 4u) || fr[q].n_bytes != n_stop * 3 * rs || fr[q].offset + per_frame > used) { rc = 19; break; }
                for (size_t z = fr[q].offset + fr[q].n_bytes; z < fr[q].offset + per_frame; z++) if (blob[z]) rc = 20;
                // the bytes are the reals of the leading atoms: unpacked here they are what the host decoded
                for (uint32_t g = 0; g < nout && !rc; g++) {
                    const uint32_t a = group.empty() ? g : group[g];
                    for (int c = 0; c < 3; c++) {
                        const uint8_t *w = &blob[fr[q].offset + (size_t)(3 * a + c) * rs];
                        uint64_t u = 0;
                        for (uint32_t z = 0; z < rs; z++) u = (u << 8) | w[z];
                        float f;
                        if (dbl) { double d; memcpy(&d, &u, 8); f = (float)d; } else { const uint32_t v = (uint32_t)u; memcpy(&f, &v, 4); }
                        if (memcmp(&f, &rx[(k * nout + g) * 3 + c], 4)) rc = 21;
                    }
                }
                // ... and gorder_xtc_read_at finds the frame again (a reader of its own: this one goes on packing)
                gorder_xtc_reader *r2 = nullptr;
                if (gorder_xtc_open(p.c_str(), group.empty() ? nullptr : group.data(), (uint32_t)group.size(), &r2)) { rc = 22; break; }
                if (gorder_xtc_read_at(r2, pos[q], one.data(), ob.data()) || memcmp(one.data(), &rx[k * nout * 3], (size_t)nout * 12)) rc = 23;
                gorder_xtc_close(r2);
            }
        }
        gorder_xtc_close(r);
        if (rc) break;
    }
    if (pool) gorder_xtc_pool_destroy(pool);
    if (!rc && (k != rt.size() || state != state_read || last != last_read)) rc = 24;
    return rc;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return fail(1, "usage: trr_pack_sanitize <directory>");
    const std::string dir = argv[1];
    std::vector<float> x(3 * N * 7);
    for (size_t k = 0; k < x.size(); k++) x[k] = (float)((k * 2654435761u % 100000u) * 1e-4 - 3.0);
    for (int d = 0; d < 2; d++) {
        const bool dbl = d != 0;
        const std::string tag = dbl ? "d" : "s";
        // 7 frames (t = 2.5 k), a velocities-only frame behind the first, frame 4 without a box; the same in two files
        std::vector<uint8_t> whole, a, b;
        std::vector<size_t> x_at;
        for (int k = 0; k < 7; k++) {
            std::vector<uint8_t> one;
            frame(one, 10 * k, 2.5 * k, k != 4, true, dbl, &x[(size_t)k * 3 * N]);
            x_at.push_back(whole.size() + one.size() - (size_t)3 * N * (dbl ? 8 : 4));
            whole.insert(whole.end(), one.begin(), one.end());
            if (k <= 3) a.insert(a.end(), one.begin(), one.end());
            if (k >= 3) b.insert(b.end(), one.begin(), one.end());
            if (k == 0) { frame(whole, 5, 1.0, true, false, dbl, x.data()); frame(a, 5, 1.0, true, false, dbl, x.data()); }
        }
        const std::string pw = dir + "/whole_" + tag + ".trr", pa = dir + "/a_" + tag + ".trr", pb = dir + "/b_" + tag + ".trr";
        if (!write_file(pw, whole, whole.size()) || !write_file(pa, a, a.size()) || !write_file(pb, b, b.size())) return fail(2, "cannot write");
        int format = -1; uint32_t na = 0, first = 0; uint64_t fb = 0;
        if (gorder_xtc_probe_format(pw.c_str(), &format, &na, &fb, &first) || format != GORDER_XTC_FORMAT_TRR || na != N ||
            fb != whole.size() || first != (dbl ? 92u : 84u) + 3 * N * (dbl ? 8u : 4u) || gorder_xtc_probe(pw.c_str(), nullptr, nullptr, nullptr) != 0)
            return fail(3, "probe");
        const std::vector<std::vector<uint32_t>> groups = {{}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19}, {3, 5, 30}, {36}, {30, 3, 5}};
        const float windows[3][3] = {{0.0f, -1.0f, 1.0f}, {2.5f, 12.5f, 2.0f}, {0.0f, -1.0f, 3.0f}};
        for (const auto &g : groups)
            for (const auto &w : windows)
                for (int pooled = 0; pooled < 2; pooled++)
                    for (int split = 0; split < 2; split++) {
                        const int rc = compare(split ? std::vector<std::string>{pa, pb} : std::vector<std::string>{pw}, g, w[0], w[1],
                                               (uint32_t)w[2], dbl, pooled != 0);
                        if (rc) return fail(rc, "pack differs from read_window");
                    }
        // a blob below one frame: NO_SPACE, nothing has happened
        {
            gorder_xtc_reader *r = nullptr;
            if (gorder_xtc_open(pw.c_str(), nullptr, 0, &r)) return fail(4, "open");
            uint64_t state = 0, used = 0; double last = -INFINITY;
            std::vector<uint8_t> blob(4096);
            std::vector<gorder_xtc_frame_t> fr(8);
            std::vector<float> bx(8 * 9), t(8);
            if (gorder_xtc_pack_window(r, 0, -1, 1, &state, &last, blob.data(), 100, &used, fr.data(), bx.data(), t.data(), 8, 2) != GORDER_XTC_ERR_NO_SPACE ||
                state != 0 || last != -INFINITY)
                return fail(5, "NO_SPACE");
            gorder_xtc_close(r);
        }
        // format errors, found before anything is copied
        const std::string pc = dir + "/cut_" + tag + ".trr", px = dir + "/xsize_" + tag + ".trr";
        std::vector<uint8_t> bad;
        frame(bad, 0, 0.0, true, true, dbl, x.data());
        frame(bad, 1, 2.5, true, true, dbl, x.data(), (long)(3 * (N - 1) * (dbl ? 8 : 4)));
        if (!write_file(pc, whole, x_at[5] + 100) || !write_file(px, bad, bad.size())) return fail(6, "cannot write");
        for (const std::string &p : {pc, px})
            for (int grp = 0; grp < 2; grp++) {
                const uint32_t two[2] = {0, 1};
                gorder_xtc_reader *r = nullptr;
                if (gorder_xtc_open(p.c_str(), grp ? two : nullptr, grp ? 2 : 0, &r)) return fail(7, "open");
                uint64_t state = 0, used = 0; double last = -INFINITY;
                std::vector<uint8_t> blob(1 << 16);
                std::vector<gorder_xtc_frame_t> fr(8);
                std::vector<float> bx(8 * 9), t(8);
                const int64_t got = gorder_xtc_pack_window(r, 0, -1, 1, &state, &last, blob.data(), blob.size(), &used, fr.data(), bx.data(), t.data(), 8, 2);
                gorder_xtc_close(r);
                if (got != GORDER_XTC_ERR_FORMAT) return fail(8, "a corrupt file was packed");
            }
        printf("%s precision ok\n", dbl ? "double" : "single");
    }
    return 0;
}
