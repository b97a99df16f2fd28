// Drives gorder_amd/csrc/replay_rows.h (the host side of the whole-trajectory manual tables) without a device: the mapping
// from frame to assignment index and table row, the rows a batch opens and the row it carries into the next, what is
// collected, the missing-row and bad-step errors, and the packing of flag bytes into words for 1, 63, 64, 65 and 129
// molecules.  Every batch plan is compared with a frame-by-frame restatement of the reference's lookup.  Built with
// -fsanitize=address,undefined by tests/test_replay_cpu.py; exit status 0 and "replay_rows ok" when everything agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "replay_rows.h"

namespace {

uint64_t rng_state = 0x2545F4914F6CDD1Dull;
uint64_t next_random() {       // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

// the handle's side of a run, reduced to what replay_rows.h decides: expanded rows by table row, row 0 = the carry
struct Run {
    uint32_t frequency;
    gorder::ReplayWindow win;
    bool have_carry = false;
    uint64_t carry_index = 0;
    std::vector<uint64_t> collected;          // frames of the collected rows
    std::vector<uint64_t> collected_index;    // ... and the table rows they came from
};

// one batch: plan it, then check every frame against the literal lookup (leaflets.rs:835-839)
int batch(Run &run, const std::vector<uint64_t> &frames) {
    gorder::ReplayLeafletBatch b;
    uint64_t bad = ~0ull;
    const gorder::ReplayStatus st = gorder::replay_plan_leaflets(run.frequency, run.win, run.have_carry, run.carry_index, frames.data(),
                                                                 (uint32_t)frames.size(), b, &bad);
    CHECK(st == gorder::kReplayOk);
    CHECK(b.arow.size() == frames.size());
    CHECK(b.collect_rows.size() == b.collect_frames.size());
    std::vector<uint64_t> row_index(b.expand.size() + 1);            // assignment index held by every expanded row
    row_index[0] = run.carry_index;
    for (size_t k = 0; k < b.expand.size(); k++) {
        CHECK((uint64_t)b.expand[k] < run.win.n_rows);
        row_index[k + 1] = run.win.first_row + b.expand[k];
    }
    for (size_t f = 0; f < frames.size(); f++) {
        const uint64_t want = run.frequency ? frames[f] / run.frequency : 0;
        CHECK(b.arow[f] <= b.expand.size());
        CHECK(b.arow[f] != 0 || run.have_carry);                      // row 0 only where there is a carry
        CHECK(row_index[b.arow[f]] == want);
        CHECK(f == 0 || b.arow[f] >= b.arow[f - 1]);                  // rows are opened in order
    }
    for (size_t k = 0; k < b.collect_rows.size(); k++) {
        CHECK(b.collect_rows[k] >= 1 && b.collect_rows[k] <= b.expand.size());
        CHECK(gorder::replay_should_assign(run.frequency, b.collect_frames[k]));
        CHECK(row_index[b.collect_rows[k]] == (run.frequency ? b.collect_frames[k] / run.frequency : 0));
        run.collected.push_back(b.collect_frames[k]);
        run.collected_index.push_back(row_index[b.collect_rows[k]]);
    }
    if (!frames.empty()) {
        CHECK(b.have_carry);
        CHECK(b.carry_index == (run.frequency ? frames.back() / run.frequency : 0));
        CHECK(b.carry_index == row_index[b.arow.back()]);
    } else {
        CHECK(b.have_carry == run.have_carry && b.carry_index == run.carry_index && b.expand.empty());
    }
    run.have_carry = b.have_carry;
    run.carry_index = b.carry_index;
    return 0;
}

std::vector<uint64_t> range(uint64_t a, uint64_t b, uint64_t step = 1) {
    std::vector<uint64_t> v;
    for (uint64_t f = a; f < b; f += step) v.push_back(f);
    return v;
}

int leaflet_cases() {
    // frequency 1: every frame opens a row, every row is collected, however the frames are cut
    for (const std::vector<uint64_t> &cuts : {std::vector<uint64_t>{0, 12}, std::vector<uint64_t>{0, 5, 6, 12}, std::vector<uint64_t>{0, 1, 2, 3, 12}}) {
        Run run{1, {0, 12}};
        for (size_t k = 0; k + 1 < cuts.size(); k++)
            if (batch(run, range(cuts[k], cuts[k + 1]))) return 1;
        CHECK(run.collected == range(0, 12));
        CHECK(run.collected_index == range(0, 12));
    }
    // frequency 3, frames 0..11: cut inside an interval (4) and on an assignment frame (9); at the end of an interval (6);
    // one frame a batch
    for (const std::vector<uint64_t> &cuts : {std::vector<uint64_t>{0, 4, 9, 12}, std::vector<uint64_t>{0, 6, 12}, std::vector<uint64_t>{0, 3, 5, 6, 12},
                                              range(0, 13)}) {
        Run run{3, {0, 4}};
        for (size_t k = 0; k + 1 < cuts.size(); k++)
            if (batch(run, range(cuts[k], cuts[k + 1]))) return 1;
        CHECK((run.collected == std::vector<uint64_t>{0, 3, 6, 9}));
        CHECK((run.collected_index == std::vector<uint64_t>{0, 1, 2, 3}));
    }
    {   // a batch that continues the carried interval opens nothing: its first frames read row 0
        Run run{3, {0, 4}};
        if (batch(run, range(0, 4))) return 1;
        gorder::ReplayLeafletBatch b;
        const std::vector<uint64_t> fr = range(4, 9);
        CHECK(gorder::replay_plan_leaflets(3, run.win, true, 1, fr.data(), 5, b, nullptr) == gorder::kReplayOk);
        CHECK((b.arow == std::vector<uint32_t>{0, 0, 1, 1, 1}) && (b.expand == std::vector<uint32_t>{2}));
        CHECK((b.collect_rows == std::vector<uint32_t>{1}) && (b.collect_frames == std::vector<uint64_t>{6}));
    }
    {   // a shard that starts between two assignment frames, nothing carried: the row is expanded again, nothing is collected
        Run run{5, {0, 3}};
        if (batch(run, range(7, 12))) return 1;
        CHECK((run.collected == std::vector<uint64_t>{10}) && (run.collected_index == std::vector<uint64_t>{2}));
        gorder::ReplayLeafletBatch b;
        const std::vector<uint64_t> fr = range(7, 10);
        CHECK(gorder::replay_plan_leaflets(5, run.win, false, 0, fr.data(), 3, b, nullptr) == gorder::kReplayOk);
        CHECK((b.arow == std::vector<uint32_t>{1, 1, 1}) && (b.expand == std::vector<uint32_t>{1}) && b.collect_rows.empty());
    }
    {   // frequency 0 (once): one row for every frame, collected at frame 0 only
        Run run{0, {0, 1}};
        if (batch(run, range(0, 5))) return 1;
        if (batch(run, range(5, 9))) return 1;
        CHECK((run.collected == std::vector<uint64_t>{0}) && run.carry_index == 0);
        Run late{0, {0, 1}};
        if (batch(late, {7, 8, (uint64_t)1 << 40})) return 1;
        CHECK(late.collected.empty());
    }
    {   // first_row > 0: a rank's window, the rows counted from it
        Run run{3, {2, 2}};                                          // assignment indices 2 and 3 = frames 6..11
        if (batch(run, range(6, 8))) return 1;
        if (batch(run, range(8, 12))) return 1;
        CHECK((run.collected == std::vector<uint64_t>{6, 9}) && (run.collected_index == std::vector<uint64_t>{2, 3}));
        gorder::ReplayLeafletBatch b;
        uint64_t bad = 0;
        const std::vector<uint64_t> before = range(4, 8), after = range(10, 14);
        CHECK(gorder::replay_plan_leaflets(3, run.win, false, 0, before.data(), 4, b, &bad) == gorder::kReplayMissingRow && bad == 4);
        CHECK(gorder::replay_plan_leaflets(3, run.win, false, 0, after.data(), 4, b, &bad) == gorder::kReplayMissingRow && bad == 12);
        // ... but a frame of the carried interval needs no row of the window
        const std::vector<uint64_t> carried = {5, 6};
        CHECK(gorder::replay_plan_leaflets(3, run.win, true, 1, carried.data(), 2, b, &bad) == gorder::kReplayOk);
        CHECK((b.arow == std::vector<uint32_t>{0, 1}) && (b.expand == std::vector<uint32_t>{0}));
    }
    {   // a table one row short
        gorder::ReplayLeafletBatch b;
        uint64_t bad = 0;
        const std::vector<uint64_t> fr = range(0, 12);
        CHECK(gorder::replay_plan_leaflets(3, {0, 3}, false, 0, fr.data(), 12, b, &bad) == gorder::kReplayMissingRow && bad == 9);
        CHECK(gorder::replay_plan_leaflets(1, {0, 11}, false, 0, fr.data(), 12, b, &bad) == gorder::kReplayMissingRow && bad == 11);
        CHECK(gorder::replay_plan_leaflets(0, {0, 0}, false, 0, fr.data(), 12, b, &bad) == gorder::kReplayMissingRow && bad == 0);
    }
    {   // frame indices beyond 2^32: nothing is truncated
        const uint64_t base = ((uint64_t)1 << 32) * 3 + 3;           // a multiple of 3
        Run run{3, {base / 3, 4}};
        if (batch(run, range(base, base + 5))) return 1;
        if (batch(run, range(base + 5, base + 12))) return 1;
        CHECK((run.collected == std::vector<uint64_t>{base, base + 3, base + 6, base + 9}));
        CHECK(run.collected_index.front() == base / 3 && run.collected_index.back() == base / 3 + 3);
        gorder::ReplayLeafletBatch b;
        uint64_t bad = 0;
        const std::vector<uint64_t> low = {3};                        // the low 32 bits of `base` alone
        CHECK(gorder::replay_plan_leaflets(3, run.win, false, 0, low.data(), 1, b, &bad) == gorder::kReplayMissingRow && bad == 3);
        const uint64_t last = ~(uint64_t)0;
        const std::vector<uint64_t> top = {last - 1, last};
        CHECK(gorder::replay_plan_leaflets(1, {last - 1, 2}, false, 0, top.data(), 2, b, &bad) == gorder::kReplayOk);
        CHECK((b.expand == std::vector<uint32_t>{0, 1}));
    }
    {   // random frequencies, windows and cuts of an ascending run of frames
        for (int round = 0; round < 200; round++) {
            const uint32_t frequency = (uint32_t)(next_random() % 6);
            const uint64_t first = next_random() % 40, n = 1 + next_random() % 60;
            const uint64_t i0 = frequency ? first / frequency : 0, i1 = frequency ? (first + n - 1) / frequency : 0;
            Run run{frequency, {i0, i1 - i0 + 1}};
            std::vector<uint64_t> want;
            for (uint64_t f = first; f < first + n; f++)
                if (gorder::replay_should_assign(frequency, f)) want.push_back(f);
            for (uint64_t at = first; at < first + n;) {
                const uint64_t len = 1 + next_random() % 9, end = at + len < first + n ? at + len : first + n;
                if (batch(run, range(at, end))) return 1;
                at = end;
            }
            CHECK(run.collected == want);
        }
    }
    return 0;
}

int normal_cases() {
    std::vector<uint32_t> rows;
    uint64_t bad = 77;
    {   // step 1 and 2, whole and in windows
        const std::vector<uint64_t> fr = range(0, 12);
        CHECK(gorder::replay_plan_normals(1, {0, 12}, fr.data(), 12, rows, &bad) == gorder::kReplayOk);
        for (uint32_t f = 0; f < 12; f++) CHECK(rows[f] == f);
        const std::vector<uint64_t> even = range(0, 24, 2);
        CHECK(gorder::replay_plan_normals(2, {0, 12}, even.data(), 12, rows, &bad) == gorder::kReplayOk);
        for (uint32_t f = 0; f < 12; f++) CHECK(rows[f] == f);
        CHECK(gorder::replay_plan_normals(2, {5, 7}, even.data() + 5, 7, rows, &bad) == gorder::kReplayOk);   // first_row > 0
        for (uint32_t f = 0; f < 7; f++) CHECK(rows[f] == f);
        CHECK(gorder::replay_plan_normals(2, {5, 7}, even.data() + 4, 8, rows, &bad) == gorder::kReplayMissingRow && bad == 8);
        CHECK(gorder::replay_plan_normals(2, {0, 11}, even.data(), 12, rows, &bad) == gorder::kReplayMissingRow && bad == 22);   // one row short
        CHECK(gorder::replay_plan_normals(1, {0, 0}, fr.data(), 12, rows, &bad) == gorder::kReplayMissingRow && bad == 0);
    }
    {   // a frame off the step; the first offending frame decides
        const std::vector<uint64_t> fr = {0, 2, 5, 6};
        CHECK(gorder::replay_plan_normals(2, {0, 4}, fr.data(), 4, rows, &bad) == gorder::kReplayBadStep && bad == 5);
        CHECK(gorder::replay_plan_normals(2, {0, 1}, fr.data(), 4, rows, &bad) == gorder::kReplayMissingRow && bad == 2);
        CHECK(gorder::replay_plan_normals(0, {0, 4}, fr.data(), 4, rows, &bad) == gorder::kReplayBadStep && bad == 0);
    }
    {   // beyond 2^32
        const uint64_t base = ((uint64_t)1 << 33) * 5 + 10;          // a multiple of 5
        const std::vector<uint64_t> fr = {base, base + 5, base + 10};
        CHECK(gorder::replay_plan_normals(5, {base / 5, 3}, fr.data(), 3, rows, &bad) == gorder::kReplayOk);
        CHECK((rows == std::vector<uint32_t>{0, 1, 2}));
        const std::vector<uint64_t> low = {10};
        CHECK(gorder::replay_plan_normals(5, {base / 5, 3}, low.data(), 1, rows, &bad) == gorder::kReplayMissingRow && bad == 10);
    }
    CHECK(gorder::replay_window_ok(0, 0) && gorder::replay_window_ok(~(uint64_t)0 - 5, 5) && !gorder::replay_window_ok(~(uint64_t)0 - 5, 6));
    CHECK(gorder::replay_window_ok(0, 0xffffffffull) && !gorder::replay_window_ok(0, 0x100000000ull));
    return 0;
}

int packing_cases() {
    for (size_t n_mol : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)129}) {
        const size_t words = gorder::replay_flag_words(n_mol);
        CHECK(words == (n_mol + 63) / 64);
        for (int round = 0; round < 8; round++) {
            // exactly n_mol bytes and exactly `words` words on the heap: a byte or a word too far is the sanitizer's
            std::vector<uint8_t> flags(n_mol);
            for (uint8_t &f : flags) f = (uint8_t)(next_random() & 1u);
            if (round == 0) flags.assign(n_mol, 1);
            if (round == 1) flags.assign(n_mol, 0);
            if (round == 2) flags.back() = 1;
            if (round == 3) { flags.back() = 0; flags[0] = 3; }           // bit 0 counts, as in gorder_hip_set_manual_leaflets
            if (round == 4) flags[0] = 2;
            std::vector<uint64_t> packed(words, ~(uint64_t)0);
            gorder::replay_pack_flags(flags.data(), n_mol, packed.data());
            if (n_mol % 64u) CHECK((packed[words - 1] >> (n_mol % 64u)) == 0);   // the bits past the last molecule are 0
            for (size_t m = 0; m < n_mol; m++) {
                CHECK(gorder::replay_flag_of(packed.data(), m, false) == (flags[m] & 1u));
                CHECK(gorder::replay_flag_of(packed.data(), m, true) == ((flags[m] & 1u) ^ 1u));
            }
        }
    }
    return 0;
}

}  // namespace

int main() {
    if (leaflet_cases() || normal_cases() || packing_cases()) return 1;
    puts("replay_rows ok");
    return 0;
}
